"""Unconditional AR-DAE score networks (ardae_cdae_desc.kind 2 / 3): layout, argument validation, module surface, and the float64
restatement of the two networks that the GPU tests lean on (tests/score_restate.py) - pinned here to the reference's fp64 fixtures.  No GPU needed."""
import ctypes

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from ardae_amd.engine_common import _FlatOpt
from score_restate import ARDAE, load, loss_and_grads, rel, score, state_dict_of

KIND_ID = ARDAE.kind_id
fixtures = ARDAE.fixtures
# parameter counts of the reference classes, (d, h, L) -> (grad, res)
REFERENCE_COUNTS = {(2, 256, 3): (132865, 133122), (32, 256, 3): (140545, 148512), (2, 64, 3): (8641, 8706), (3, 100, 2): (10701, 10903)}


# ---- 1. layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_layout_totals_match_c_side_and_reference_counts(kind):
    for (d, h, nl), counts in REFERENCE_COUNTS.items():
        total = layout.offsets(layout.dae_spec(kind, d, h, nl))[1]
        desc = L.CdaeDesc(KIND_ID[kind], d, 0, h, nl, L.ACT["softplus"])
        assert total == L.query("ardae_cdae_param_floats", desc) == counts[kind == "res"]
        assert L.query("ardae_cdae_packed_floats", desc) > total
        assert L.query("ardae_cdae_workspace_floats", desc, 16, 4, 1) > L.query("ardae_cdae_workspace_floats", desc, 16, 4, 0) > 0
        assert L.query("ardae_cdae_workspace_floats", desc, 16, 4, 1) == L.query("ardae_cdae_workspace_floats", desc, 64, 1, 1)    # N = B S in any factorisation


def test_layout_names_and_shapes_are_the_fixtures(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        (_, d, h, nl), kind = (int(v) for v in fx["shape"]), str(fx["kind"])
        sd = state_dict_of(fx)
        assert [(n, tuple(s)) for n, s in layout.dae_spec(kind, d, h, nl)] == [(k, tuple(v.shape)) for k, v in sd.items()], path


# ---- 2. validation before any HIP call ---------------------------------------------------------------------------------------------
def test_argument_validation_of_the_unconditional_entry_points():
    lib = L.lib()
    one, big = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40)      # any non-null address: validation must fail before it is dereferenced

    def fails(rc, fragment):
        assert rc < 0
        assert fragment.encode() in lib.ardae_last_error(), lib.ardae_last_error()

    ok = L.CdaeDesc(2, 2, 0, 64, 3, 2)
    ref = ctypes.byref
    for bad, fragment in ((L.CdaeDesc(2, 2, 1, 64, 3, 2), "context_dim must be 0"), (L.CdaeDesc(3, 2, 2, 64, 3, 2), "context_dim must be 0"),
                          (L.CdaeDesc(0, 2, 0, 64, 3, 2), "context_dim >= 1"), (L.CdaeDesc(1, 2, 0, 64, 3, 2), "context_dim >= 1"),
                          (L.CdaeDesc(4, 2, 0, 64, 3, 2), "kind must be")):
        assert lib.ardae_cdae_param_floats(ref(bad)) == lib.ardae_cdae_packed_floats(ref(bad)) == lib.ardae_cdae_workspace_floats(ref(bad), 4, 8, 1) == 0
        fails(lib.ardae_cdae_pack(ref(bad), one, one, None), fragment)
        fails(lib.ardae_cdae_loss_grads(ref(bad), one, one, one, one, one, None, 4, 8, one, big, one, one, None, None), fragment)
        fails(lib.ardae_cdae_score(ref(bad), one, one, one, one, None, 4, 8, one, big, one, None), fragment)
        assert lib.ardae_dae_perturb_fused_ok(ref(bad), 10) == 0
    # a context pointer is an error for the unconditional kinds, not ignored
    fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, one, 4, 8, one, big, one, one, None, None), "ctx must be NULL")
    fails(lib.ardae_cdae_score(ref(ok), one, one, one, one, one, 4, 8, one, big, one, None), "ctx must be NULL")
    fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, None, one, one, None, 4, 8, one, big, one, one, None, None), "null pointer")
    fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, None, 0, 8, one, big, one, one, None, None), "bad batch")
    fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, None, 4, 8, one, ctypes.c_size_t(16), one, one, None, None), "workspace too small")
    # the perturbation and the fused front end
    fails(lib.ardae_dae_perturb(None, one, one, 4, 8, 2, one, None), "null pointer")
    fails(lib.ardae_dae_perturb(one, one, one, 0, 8, 2, one, None), "bad batch")
    fails(lib.ardae_dae_perturb(one, one, one, 4, 0, 2, one, None), "bad batch")
    fused = lambda desc, x, B, ns, first, ws: lib.ardae_dae_perturb_loss_grads(ref(desc), one, one, x, B, ns, 1.0, 7, 0, 1, None, first, one, one, one, one,
                                                                                ws, one, one, None)
    fails(fused(ok, None, 4, 8, 0, big), "null pointer")
    fails(fused(ok, one, 0, 8, 0, big), "bad batch")
    fails(fused(ok, one, 4, 0, 0, big), "bad batch")
    fails(fused(ok, one, 4, 8, 2, big), "first_row must be a multiple of 4")
    fails(fused(ok, one, 4, 8, 0, ctypes.c_size_t(16)), "workspace too small")
    fails(fused(L.CdaeDesc(2, 3, 0, 100, 2, 3), one, 4, 8, 0, big), "not eligible")
    fails(fused(L.CdaeDesc(0, 2, 2, 64, 3, 2), one, 4, 8, 0, big), "not eligible")


def test_fused_front_end_eligibility_answers_without_a_device():
    okq = lambda kind, d, h, nl, act, ns: L.query("ardae_dae_perturb_fused_ok", L.CdaeDesc(kind, d, 0, h, nl, L.ACT[act]), ns)
    for kind in (2, 3):
        assert okq(kind, 2, 256, 3, "softplus", 10) == 1      # ardae_fit.ipynb: 1024 x 10 rows, h 256
        assert okq(kind, 2, 128, 3, "softplus", 10) == 1      # ardae_toy.ipynb: 256 x 10 rows, h 128
        assert okq(kind, 3, 100, 2, "elu", 10) == 0           # h is not 64 | 128 | 256
        assert okq(kind, 32, 256, 3, "softplus", 10) == 0     # d > 8
        assert okq(kind, 2, 64, 1, "relu", 10) == 0           # a single layer also seeds the score pass
        assert okq(kind, 2, 256, 3, "softplus", 0) == 0
    assert L.query("ardae_dae_perturb_fused_ok", L.CdaeDesc(0, 2, 2, 256, 3, 2), 10) == 0
    assert L.query("ardae_cdae_perturb_fused_ok", L.CdaeDesc(2, 8, 0, 256, 3, 2), 256, 1) == 0   # the conditional front end refuses kinds 2 / 3


# ---- 3. modules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,names", [(net.MLPGradARDAE, ["neglogprob.layers.0.weight", "neglogprob.layers.0.bias", "neglogprob.fc.weight", "neglogprob.fc.bias"]),
                                       (net.MLPResARDAE, ["main.layers.0.weight", "main.layers.0.bias", "main.fc.weight", "main.fc.bias"])])
def test_module_defaults_are_the_references(cls, names):
    m = cls()
    assert (m.input_dim, m.h_dim, m.std, m.num_hidden_layers, m.nonlinearity, m.noise_type) == (2, 1000, 0.1, 1, "tanh", "gaussian")
    assert [n for n, _ in m.named_parameters()] == names
    assert m.state_dict()[names[0]].shape == (1000, 3)
    assert int(m._desc.kind) == (2 if cls is net.MLPGradARDAE else 3) and int(m._desc.context_dim) == 0
    with pytest.raises(NotImplementedError):
        cls(noise_type="laplace")
    with pytest.raises(NotImplementedError):
        cls(nonlinearity="gelu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16)(torch.zeros(4, 2), torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16).glogprob(torch.zeros(4, 2))


def test_load_state_dict_keeps_flat_views(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        (_, d, h, nl), kind = (int(v) for v in fx["shape"]), str(fx["kind"])
        m = (net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=str(fx["act"]))
        sd = state_dict_of(fx)
        m.load_state_dict(sd)
        off = 0
        for n, p in m.named_parameters():
            assert p.data_ptr() == m.flat_params().data_ptr() + 4 * off and torch.equal(p, sd[n])
            off += p.numel()
        assert off == m.flat_params().numel() == L.query("ardae_cdae_param_floats", m._desc)


def test_score_engine_refuses_other_networks_and_bad_batches():
    import types
    ArdaeScoreEngine = net.ArdaeScoreEngine
    eng = types.SimpleNamespace(B=4, d=2, dev=torch.device("cuda", 0))
    check = lambda x: ArdaeScoreEngine._check_batch(eng, x, "step(x)")
    with pytest.raises(ValueError, match="on cuda:0"):
        check(torch.zeros(4, 2))                      # host batch
    with pytest.raises(ValueError, match="batch_size=4"):
        check(torch.zeros(3, 2))
    with pytest.raises(ValueError, match="batch_size=4"):
        check(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="contiguous"):
        check(torch.zeros(4, 4)[:, ::2])
    with pytest.raises(ValueError, match="float32"):
        check(torch.zeros(4, 2).double())
    with pytest.raises(TypeError):
        check([[0.0, 0.0]] * 4)
    assert ArdaeScoreEngine.RNG_STRIDE * 1000 + 1 < net.rng.HOST_STREAM


# ---- 4. the float64 restatement reproduces every fp64 fixture ----------------------------------------------------------------------
def test_restatement_reproduces_the_fp64_fixtures(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        kind, act = str(fx["kind"]), str(fx["act"])
        p = {k: v.double() for k, v in state_dict_of(fx).items()}
        x, std, eps = (torch.tensor(fx[k]).double() for k in ("x", "std", "eps"))
        loss, grads = loss_and_grads(kind, p, act, x, std, eps, True)
        assert abs(float(loss) - float(fx["loss64"])) <= 1e-12 * abs(float(fx["loss64"])), path
        for n, g in grads.items():
            if f"g64/{n}/none" in fx:
                assert g is None, (path, n)
            else:
                assert rel(g, fx["g64/" + n]) <= 1e-12, (path, n, rel(g, fx["g64/" + n]))
        assert rel(score(kind, p, act, x, torch.zeros_like(std)), fx["glog0_64"]) <= 1e-12, path
        assert rel(score(kind, p, act, x, std), fx["glog_64"]) <= 1e-12, path


# ---- 5. host logic the engines share (engine_common.py): per-parameter views, the optimiser's checkpoint ---------------------------
def test_param_views_alias_the_parameters_and_name_the_tensor_without_gradient():
    mods = [net.MLPGradARDAE(input_dim=3, h_dim=16, num_hidden_layers=2, nonlinearity="elu"),
            net.MLPGradCARDAE(input_dim=4, context_dim=4, h_dim=16, num_hidden_layers=2, nonlinearity="softplus"),
            net.MLPResCARDAE(input_dim=4, context_dim=4, h_dim=16, num_hidden_layers=2, nonlinearity="softplus"),
            net.Generator(hidden_dim=16, z_dim=3, num_hidden_layers=2),
            net.MNISTIPVAE(input_dim=24, noise_dim=6, h_dim=16, z_dim=4, num_hidden_layers=1, nonlinearity="softplus", enc_type="concat")]
    for m in mods:
        flat, params = m.flat_params(), list(m.named_parameters())
        views = m.param_views(flat)
        assert len(views) == len(params) and sum(v.numel() for v in views) == flat.numel()
        for v, (name, p) in zip(views, params):
            assert v.data_ptr() == p.data_ptr() and v.shape == p.shape, name
        other = torch.zeros_like(flat)                      # any buffer of that layout, not the parameters alone
        assert [v.data_ptr() - other.data_ptr() for v in m.param_views(other)] == [v.data_ptr() - flat.data_ptr() for v in views]
        grad_kind = isinstance(m, (net.MLPGradARDAE, net.MLPGradCARDAE))
        assert set(m._no_grad_names) == ({"neglogprob.fc.bias"} if grad_kind else set())
        masked = m.param_views(flat, grads_only=True)
        assert [v is None for v in masked] == [name in m._no_grad_names for name, _ in params]
        assert all(v is None or v.data_ptr() == w.data_ptr() for v, w in zip(masked, views))
        if grad_kind:
            # it is the LAST tensor of the layout: "the first numel - 1 floats" (_FlatOpt.n, a kernel argument) and the name set say the same
            assert params[-1][0] == "neglogprob.fc.bias" and m._offs["neglogprob.fc.bias"][:2] == (flat.numel() - 1, 1)
            assert sum(v.numel() for v in masked if v is not None) == flat.numel() - 1


def _flat_opt(kind, seed=0):
    torch.manual_seed(seed)
    m = net.MLPGradARDAE(input_dim=3, h_dim=16, num_hidden_layers=2, nonlinearity="elu")
    return m, _FlatOpt(kind, m.flat_params(), m.flat_params().numel() - 1, 1e-3, 0.5, 0.5)        # construction launches nothing


def _filled(kind):
    m, opt = _flat_opt(kind)
    opt.steps = 3
    for k, b in enumerate(opt.buffers()):
        b.copy_(torch.arange(b.numel()) + 10000.0 * (k + 1))
    return m, opt


@pytest.mark.parametrize("kind", ["sgd", "rmsprop", "adam", "amsgrad"])
def test_flat_opt_state_dict_has_torchs_layout_and_round_trips(kind):
    m, opt = _filled(kind)
    assert opt.n == m.flat_params().numel() - len(m._no_grad_names)
    sd = opt.state_dict(m)
    assert list(sd) == ["state", "param_groups"]
    params = [p for _, p in m.named_parameters()]
    ref = {"sgd": lambda: torch.optim.SGD(params, lr=1e-3), "rmsprop": lambda: torch.optim.RMSprop(params, lr=1e-3, momentum=0.5),
           "adam": lambda: torch.optim.Adam(params, lr=1e-3, betas=(0.5, 0.999)),
           "amsgrad": lambda: torch.optim.Adam(params, lr=1e-3, betas=(0.5, 0.999), amsgrad=True)}[kind]()
    g = torch.Generator().manual_seed(1)
    for name, p in m.named_parameters():
        p.grad = None if name in m._no_grad_names else torch.randn(p.shape, generator=g)
    ref.step()
    want = ref.state_dict()
    assert list(sd["state"]) == list(want["state"]) == ([] if kind == "sgd" else list(range(len(params) - 1)))      # no entry for the bias
    for i, st in sd["state"].items():
        assert list(st) == list(want["state"][i]) == ["step"] + list(opt.state_names())
        assert st["step"] == 3 and all(st[k].shape == params[i].shape for k in opt.state_names())
    assert set(sd["param_groups"][0]) <= set(want["param_groups"][0]) and sd["param_groups"][0]["params"] == want["param_groups"][0]["params"]
    assert len(sd["param_groups"]) == len(want["param_groups"]) == 1
    # into a second optimiser over a fresh module
    m2, opt2 = _flat_opt(kind, seed=1)
    for b in opt2.buffers():
        b.fill_(-1.0)
    assert opt2.load_state_dict(m2, sd, "checkpoint") == (0 if kind == "sgd" else 3)
    assert len(opt2.buffers()) == len(opt.buffers()) == len(opt.state_names())
    for a, b in zip(opt.buffers(), opt2.buffers()):
        assert torch.equal(a[:opt.n], b[:opt.n]) and float(b[opt.n:].abs().sum()) == 0.0      # the bias keeps no state
    assert opt2.state_dict(m2)["state"] == {} and opt2.steps == 0                                    # the step count is the caller's to set
    opt2.steps = 3
    again = opt2.state_dict(m2)
    assert all(torch.equal(again["state"][i][k], sd["state"][i][k]) for i in sd["state"] for k in opt.state_names())


def test_flat_opt_refuses_foreign_and_inconsistent_state():
    m, rms = _filled("rmsprop")
    sd = rms.state_dict(m)
    _, adam = _flat_opt("adam")
    with pytest.raises(ValueError, match="written by optimiser 'rmsprop', but this engine was built with 'adam'"):
        adam.load_state_dict(m, sd, "checkpoint")
    with pytest.raises(ValueError, match="does not belong to 'adam'"):
        adam.load_state_dict(m, {"state": sd["state"]}, "checkpoint")                                 # no param_groups: the state's own keys
    sd["state"][1]["step"] = 4
    with pytest.raises(ValueError, match=r"one step count per network \(checkpoint: \[3, 4\]\)"):
        rms.load_state_dict(m, sd, "checkpoint")
