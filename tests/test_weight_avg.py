"""--m-weight-avg (ivae_ardae.py:158-164,559-565) without a GPU: configuration checks, the wrappers' argument checks and the pure-Python
conversion between the plain and the wrapped optimiser checkpoint layouts (optim.py, "Weight averaging")."""
import ctypes
import io

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import optim


def test_train_config_weight_avg_fields():
    cfg = net.TrainConfig()
    assert (cfg.m_weight_avg, cfg.m_weight_avg_start, cfg.m_weight_avg_decay, cfg.m_weight_avg_freq) == ("none", 1000, 0.998, 1)
    for kind in ("none", "swa", "polyak"):
        net.TrainConfig(m_weight_avg=kind)
    with pytest.raises(NotImplementedError):
        net.TrainConfig(m_weight_avg="ema")
    with pytest.raises(NotImplementedError):
        net.TrainConfig(m_weight_avg="polyak", m_weight_avg_freq=2)
    with pytest.raises(ValueError):
        net.TrainConfig(m_weight_avg="polyak", m_weight_avg_decay=1.5)
    with pytest.raises(ValueError):
        net.TrainConfig(m_weight_avg="swa", m_weight_avg_start=-1)


def _tiny_model():
    return net.MNISTIPVAE(input_dim=24, noise_dim=10, h_dim=32, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=8)


def test_wrappers_refuse_what_is_not_implemented():
    opt = net.Adam(_tiny_model().parameters(), lr=1e-4, betas=(0.5, 0.999))
    with pytest.raises(NotImplementedError):
        net.Polyak(opt, polyak_start=10, polyak_freq=2, polyak_decay=0.99)
    with pytest.raises(NotImplementedError):
        net.SWA(opt, swa_start=10, swa_freq=5)
    with pytest.raises(NotImplementedError):
        net.SWA(opt, swa_start=10, swa_lr=0.05)
    with pytest.raises(ValueError):
        net.Polyak(opt, polyak_start=None)
    w = net.Polyak(opt, polyak_start=10, polyak_decay=0.99)
    assert w.param_groups is opt.param_groups
    assert (w.param_groups[0]["n_avg"], w.param_groups[0]["step_counter"]) == (0, 0)
    assert net.SWA(opt, 3).kind == "swa"


@pytest.mark.parametrize("kind", ["swa", "polyak"])
def test_checkpoint_layout_round_trip(kind):
    inner = {"state": {0: {"step": 25, "exp_avg": torch.randn(3, 2), "exp_avg_sq": torch.rand(3, 2)},
                       1: {"step": 25, "exp_avg": torch.randn(3), "exp_avg_sq": torch.rand(3)}},
             "param_groups": [{"lr": 1e-4, "betas": (0.5, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "params": [0, 1],
                               "n_avg": 15, "step_counter": 25}]}
    bufs = {0: torch.randn(3, 2), 1: torch.randn(3)}
    sd = optim.wrap_state_dict(inner, kind, bufs)
    skey, bkey = optim.weight_avg_keys(kind)
    assert sorted(sd) == sorted(["opt_state", skey, "param_groups"])
    assert sd["opt_state"] is inner["state"] and sd[skey][1][bkey] is bufs[1]
    # survives a file read back with weights_only=True
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    back = torch.load(f, weights_only=True)
    got, got_kind, got_bufs = optim.unwrap_state_dict(back)
    assert got_kind == kind and sorted(got) == ["param_groups", "state"]
    assert got["param_groups"][0]["n_avg"] == 15 and got["param_groups"][0]["step_counter"] == 25
    assert all(torch.equal(got_bufs[i], bufs[i]) for i in bufs)
    assert torch.equal(got["state"][0]["exp_avg"], inner["state"][0]["exp_avg"])
    # a plain state_dict passes through untouched
    plain, k, b = optim.unwrap_state_dict(inner)
    assert plain is inner and k is None and b == {}
    # before the first averaging step a wrapped state carries no buffers
    empty = optim.wrap_state_dict(inner, kind, {})
    assert optim.unwrap_state_dict(empty)[2] == {}


def test_checkpoint_layout_errors():
    with pytest.raises(NotImplementedError):
        optim.wrap_state_dict({"state": {}, "param_groups": []}, "ema", {})
    with pytest.raises(ValueError):
        optim.unwrap_state_dict({"opt_state": {}, "swa_state": {}, "polyak_state": {}, "param_groups": []})
    with pytest.raises(ValueError):
        optim.unwrap_state_dict({"opt_state": {}, "param_groups": []})


def test_weight_avg_entry_declared_and_bound():
    assert "ardae_weight_avg" in L.EXPORTS
    h = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(h, "ardae_weight_avg")
    lib = L.lib()
    # argument validation happens before any HIP call
    assert lib.ardae_weight_avg(None, None, 4, 1, 0.99, 1, None, 1, None) < 0
    assert b"weight_avg" in lib.ardae_last_error()
    buf = (ctypes.c_float * 8)()
    a, p = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(ctypes.addressof(buf) + 8)
    assert lib.ardae_weight_avg(a, p, 4, 1, 0.99, 1, None, 1, None) < 0            # overlapping avg / p
    assert b"overlap" in lib.ardae_last_error()
    assert lib.ardae_weight_avg(a, p, 1, 2, 0.99, 1, None, 1, None) < 0            # unknown kind
    assert lib.ardae_weight_avg(a, p, 1, 1, 0.99, 0, None, 1, None) < 0            # origin is a step number >= 1
