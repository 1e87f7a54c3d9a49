"""Conditional AR-DAE without an input encoder (ardae_cdae_desc.kind 16 / 17; ConditionalARDAE(enc_input=False)): layout, sizes, argument
validation, module surface, and the float64 restatement the GPU tests lean on (tests/noenc_restate.py) - pinned here to the reference's fp64
fixtures.  No GPU needed."""
import ctypes
import math
import os

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from noenc_restate import NOENC, grads_on_xbar, score
from score_restate import dims, inputs_of, load, rel, state_dict_of

KIND_ID = NOENC.kind_id
SHAPES = [(2, 2, 64, 3), (3, 5, 100, 2), (32, 32, 256, 3), (2, 2, 64, 1)]      # (d, c, h, L)


# ---- 1. layout and sizes -----------------------------------------------------------------------------------------------------------
def test_layout_names_and_shapes_are_the_fixtures(golden_dir):
    for path in NOENC.fixtures(golden_dir):
        fx = load(path)
        (_, _, d, c, h, nl), kind = dims(fx), str(fx["kind"])
        sd = state_dict_of(fx)
        spec = layout.cdae_spec(kind, d, c, h, nl, enc_input=False)
        assert [(n, tuple(s)) for n, s in spec] == [(k, tuple(v.shape)) for k, v in sd.items()], path
        assert not any(n.startswith("inp_encode.") for n, _ in spec)
        assert dict(spec)[NOENC.last[kind] + "layers.0.weight"] == (h, d + h + 1)
        assert layout.offsets(spec)[1] == sum(v.numel() for v in sd.values()) == L.query("ardae_cdae_param_floats", L.CdaeDesc(KIND_ID[kind], d, c, h, nl, 2))
        assert fx["std"].shape == (int(fx["shape"][0]), int(fx["shape"][1]), 1)                        # always a tensor: ConditionalARDAE asserts one
    for kind in ("grad", "res"):
        fx = load(os.path.join(golden_dir, f"cardae_noenc_traj_{kind}.npz"))
        spec = layout.cdae_spec(kind, int(fx["cfg/d"]), int(fx["cfg/c"]), int(fx["cfg/h"]), int(fx["cfg/L"]), enc_input=False)
        assert [(n, tuple(s)) for n, s in spec] == [(k, tuple(v.shape)) for k, v in state_dict_of(fx).items()]
    # the default keeps every existing result
    assert layout.cdae_spec("grad", 2, 3, 64, 2) == layout.cdae_spec("grad", 2, 3, 64, 2, enc_input=True) == layout.cdae_spec("grad", 2, 3, 64, 2, True)
    assert dict(layout.cdae_spec("res", 2, 3, 64, 2))["dae.layers.0.weight"] == (64, 129)
    with pytest.raises(NotImplementedError):
        layout.cdae_spec("mlp", 2, 2, 64, 3, enc_input=False)


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("d,c,h,nl", SHAPES, ids=[f"d{s[0]}-c{s[1]}-h{s[2]}-L{s[3]}" for s in SHAPES])
def test_sizes(kind, d, c, h, nl):
    desc = L.CdaeDesc(KIND_ID[kind], d, c, h, nl, L.ACT["softplus"])
    sib = L.CdaeDesc(KIND_ID[kind] - 16, d, c, h, nl, L.ACT["softplus"])
    total = layout.offsets(layout.cdae_spec(kind, d, c, h, nl, enc_input=False))[1]
    assert L.query("ardae_cdae_param_floats", desc) == total
    # the sibling has the input encoder on top, and W1a [h, h] in the place of W1x [h, d]
    enc = layout.offsets(layout._mlp("inp_encode.", d, h, h, nl - 1))[1]
    assert L.query("ardae_cdae_param_floats", sib) == total + enc + h * (h - d)
    assert 0 < L.query("ardae_cdae_packed_floats", desc) < L.query("ardae_cdae_packed_floats", sib)
    for B, S in ((4, 8), (3, 256)):
        w0, w1 = (L.query("ardae_cdae_workspace_floats", desc, B, S, g) for g in (0, 1))
        assert 0 < w0 < w1
        assert w0 < L.query("ardae_cdae_workspace_floats", sib, B, S, 0) and w1 < L.query("ardae_cdae_workspace_floats", sib, B, S, 1)


# ---- 2. validation before any HIP call ---------------------------------------------------------------------------------------------
def test_argument_validation():
    lib = L.lib()
    one, big = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40)      # any non-null address: validation must fail before it is dereferenced
    ref = ctypes.byref

    def fails(rc, fragment):
        assert rc < 0
        assert fragment.encode() in lib.ardae_last_error(), lib.ardae_last_error()

    for k in (16, 17):
        ok = L.CdaeDesc(k, 2, 2, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(ok)) > 0 and lib.ardae_cdae_packed_floats(ref(ok)) > 0 and lib.ardae_cdae_workspace_floats(ref(ok), 4, 8, 1) > 0
        bad = L.CdaeDesc(k, 2, 0, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(bad)) == lib.ardae_cdae_packed_floats(ref(bad)) == lib.ardae_cdae_workspace_floats(ref(bad), 4, 8, 1) == 0
        fails(lib.ardae_cdae_pack(ref(bad), one, one, None), "context_dim >= 1")
        fails(lib.ardae_cdae_loss_grads(ref(bad), one, one, one, one, one, one, 4, 8, one, big, one, one, None, None), "context_dim >= 1")
        fails(lib.ardae_cdae_score(ref(bad), one, one, one, one, one, 4, 8, one, big, one, None), "context_dim >= 1")
        # NULL ctx / sigma / xbar: the AR-DAE kinds' score reads sigma too
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, None, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, None, one, one, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, None, one, one, one, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, one, None, 4, 8, one, big, one, None), "null pointer")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, None, one, 4, 8, one, big, one, None), "null pointer")
        fails(lib.ardae_cdae_score(ref(ok), one, one, None, one, one, 4, 8, one, big, one, None), "null pointer")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, one, one, 4, 8, one, big, None, None), "score_out is NULL")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, one, 0, 8, one, big, one, one, None, None), "bad batch")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, one, 4, 8, one, ctypes.c_size_t(16), one, one, None, None), "workspace too small")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, one, one, 4, 8, one, ctypes.c_size_t(16), one, None), "workspace too small")
        # the fused front end: eligibility is a statement about shapes
        wide = L.CdaeDesc(k, 32, 32, 256, 3, 2)
        assert lib.ardae_cdae_perturb_fused_ok(ref(wide), 256, 1) == 1
        assert lib.ardae_cdae_perturb_fused_ok(ref(wide), 256, 2) == 0                                           # nstd = 2
        assert lib.ardae_cdae_perturb_fused_ok(ref(L.CdaeDesc(k, 3, 32, 256, 3, 2)), 256, 1) == 0                # z = 3
        assert lib.ardae_cdae_perturb_fused_ok(ref(wide), 20, 1) == 0                                            # nz = 20
        assert lib.ardae_cdae_perturb_fused_ok(ref(L.CdaeDesc(k, 32, 32, 256, 3, L.ACT["tanh"])), 256, 1) == 0
        assert lib.ardae_cdae_perturb_fused_ok(ref(L.CdaeDesc(k, 32, 32, 100, 3, 2)), 256, 1) == 0              # h % 32
        # ... and the same as the sibling's, shape by shape
        for z, h, nz, nstd in ((32, 256, 256, 1), (8, 64, 64, 1), (8, 64, 128, 1), (16, 64, 32, 1), (64, 128, 64, 1), (128, 128, 64, 1), (32, 256, 256, 3)):
            assert lib.ardae_cdae_perturb_fused_ok(ref(L.CdaeDesc(k, z, 4, h, 2, 2)), nz, nstd) == lib.ardae_cdae_perturb_fused_ok(ref(L.CdaeDesc(k - 16, z, 4, h, 2, 2)), nz, nstd)

        def front(desc, nz, ctx=one, ws=big, xbar=one):
            return lib.ardae_cdae_perturb_loss_grads(ref(desc), one, one, one, one, ctx, 4, nz, 1.0, 0.1, 7, 0, 1, None, 0, xbar, one, one, one, one, ws, one, one, None)
        fails(front(ok, 256), "not eligible")
        fails(front(wide, 20), "not eligible")
        fails(front(wide, 256, ws=ctypes.c_size_t(16)), "workspace too small")
        fails(front(wide, 256, ctx=None), "null pointer")
        fails(front(wide, 256, xbar=None), "null pointer")
    for k in (4, 5, 8, 9, 12, 14, 15, 18, -1):
        bad = L.CdaeDesc(k, 2, 2, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(bad)) == 0
        fails(lib.ardae_cdae_pack(ref(bad), one, one, None), "kind must be")
    assert lib.ardae_abi_version() == 1


# ---- 3. the restatement is the reference --------------------------------------------------------------------------------------------
def test_restatement_equals_the_float64_fixtures(golden_dir):
    for path in NOENC.fixtures(golden_dir):
        fx = NOENC.fixture(golden_dir, os.path.basename(path)[len("cardae_noenc_"):-len(".npz")])
        (B, S, d, c, h, nl), kind, act = dims(fx), str(fx["kind"]), str(fx["act"])
        p = {k: v.double() for k, v in state_dict_of(fx).items()}
        x, ctx, eps = inputs_of(fx, torch.float64)
        std = torch.tensor(fx["std"]).double()
        loss, grads = grads_on_xbar(kind, p, act, x + std * eps, std, eps, ctx, S)
        assert abs(float(loss) - float(fx["loss_f64"])) <= 1e-12 * abs(float(fx["loss_f64"])), path
        for n, g in grads.items():
            if g is None:
                assert f"g_f64/{n}/none" in fx and n == "neglogprob.fc.bias"
            else:
                assert rel(g, fx[f"g_f64/{n}"]) <= 1e-12, (path, n)
        assert rel(score(kind, p, act, x, torch.zeros_like(std), ctx, S).detach(), fx["glog0_f64"].reshape(B * S, d)) <= 1e-12
        assert rel(score(kind, p, act, x, std, ctx, S).detach(), fx["glog_f64"].reshape(B * S, d)) <= 1e-12


# ---- 4. modules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_module_defaults_are_the_references(kind, golden_dir):
    cls = {"grad": net.MLPGradCARDAE, "res": net.MLPResCARDAE}[kind]
    last = "neglogprob" if kind == "grad" else "dae"
    names = ["ctx_encode.fc.weight", "ctx_encode.fc.bias", f"{last}.layers.0.weight", f"{last}.layers.0.bias", f"{last}.fc.weight", f"{last}.fc.bias"]
    m = cls(enc_input=False)
    assert (m.input_dim, m.h_dim, m.context_dim, m.std, m.num_hidden_layers, m.nonlinearity, m.noise_type, m.enc_input, m.enc_ctx) == \
        (2, 128, 2, 0.01, 1, "tanh", "gaussian", False, True)
    assert [n for n, _ in m.named_parameters()] == names == list(m.state_dict())
    assert m.state_dict()[names[2]].shape == (128, 2 + 128 + 1)                # [W1x | W1c | w1s]
    assert int(m._desc.kind) == KIND_ID[kind] and int(m._desc.context_dim) == 2
    assert int(cls()._desc.kind) == KIND_ID[kind] - 16 and cls().enc_input is True          # the default is untouched
    assert set(m._no_grad_names) == ({"neglogprob.fc.bias"} if kind == "grad" else set())
    # nn.Linear's default init, which the reference constructor leaves in place: U(+-1/sqrt(fan_in)) for weight and bias, filling the range
    torch.manual_seed(3)
    m = cls(input_dim=3, context_dim=5, h_dim=100, num_hidden_layers=2, nonlinearity="elu", enc_input=False)
    fx = load(os.path.join(golden_dir, f"cardae_noenc_{kind}_b5_s12_d3_elu.npz"))
    sd_ref, sd = state_dict_of(fx), m.state_dict()
    assert [(k, v.shape) for k, v in sd.items()] == [(k, v.shape) for k, v in sd_ref.items()]
    for k, v in sd.items():
        bound = 1.0 / math.sqrt(sd[k[:-len("bias")] + "weight"].shape[1] if k.endswith("bias") else v.shape[1])
        for t in (v, sd_ref[k]):
            assert float(t.abs().max()) <= bound and (t.numel() < 50 or float(t.abs().max()) > 0.9 * bound), k
    with pytest.raises(NotImplementedError, match="enc_ctx"):
        cls(enc_input=False, enc_ctx=False)
    with pytest.raises(NotImplementedError, match="enc_ctx"):
        cls(enc_ctx=False)
    for bad in (dict(noise_type="laplace"), dict(noise_type="uniform"), dict(nonlinearity="gelu")):
        with pytest.raises(NotImplementedError):
            cls(enc_input=False, **bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16, enc_input=False)(torch.zeros(4, 3, 2), torch.zeros(4, 1, 2), torch.zeros(4, 3, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16, enc_input=False).glogprob(torch.zeros(4, 3, 2), torch.zeros(4, 1, 2))


def test_load_state_dict_keeps_flat_views(golden_dir):
    for path in NOENC.fixtures(golden_dir):
        fx = load(path)
        _, _, d, c, h, nl = dims(fx)
        m = NOENC.module(str(fx["kind"]), d, h, nl, str(fx["act"]), c)
        sd = state_dict_of(fx)
        m.load_state_dict(sd)
        again = NOENC.module(str(fx["kind"]), d, h, nl, str(fx["act"]), c)
        again.load_state_dict(m.state_dict())                                  # the round trip
        off = 0
        for (n, p), (_, q) in zip(m.named_parameters(), again.named_parameters()):
            assert p.data_ptr() == m.flat_params().data_ptr() + 4 * off and torch.equal(p, sd[n]) and torch.equal(q, sd[n])
            assert q.data_ptr() == again.flat_params().data_ptr() + 4 * off
            off += p.numel()
        assert off == m.flat_params().numel() == L.query("ardae_cdae_param_floats", m._desc)


def test_engines_take_the_new_kinds_and_keep_their_refusals():
    """Construction-time checks only: nothing here reaches the device."""
    class OnDevice:                      # the check comes right after _require_gpu(): no device is touched before it
        def __init__(self, m):
            self._desc, self._require_gpu = m._desc, lambda: None
    assert net.ArdaeCondScoreEngine._AR_KINDS == (0, 1, 16, 17)
    for cls in (net.MLPGradCARDAE, net.MLPResCARDAE):
        with pytest.raises(TypeError, match="(?s)ScoreConfig.*DaeConfig"):
            net.ArdaeCondScoreEngine(OnDevice(cls(h_dim=16, enc_input=False)), net.DaeConfig(), 4, 8)
        with pytest.raises(TypeError, match="unconditional"):
            net.ArdaeScoreEngine(OnDevice(cls(h_dim=16, enc_input=False)), net.ScoreConfig(), 4)
