"""--beta-init / --beta-annealing (ivae_ardae.py:202-203,704) without a GPU: the configuration rules and the binding of the entry
points that carry beta through the device step block (`ardae_train_state_advance` and the `_dev` twins)."""
import ctypes
import os

import pytest

import ardae_amd as net
from ardae_amd import _lib as L

vp, i32, i64, u64, f32, f64, usize = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double,
                                      ctypes.c_size_t)


def test_train_config_beta_schedule_fields():
    cfg = net.TrainConfig()
    assert (cfg.beta, cfg.beta_init, cfg.beta_annealing) == (1.0, None, None) and cfg.beta_schedule() is None
    # ivae_ardae.py:202-203: None or anything below 1 is "no annealing" (the recipes without a schedule pass 0), with or without beta_init
    for ann in (None, 0, -1):
        assert net.TrainConfig(beta_annealing=ann).beta_schedule() is None
        assert net.TrainConfig(beta_init=1e-4, beta_annealing=ann).beta_schedule() is None
    cfg = net.TrainConfig(beta=1.0, beta_init=1e-4, beta_annealing=50000)          # run_vae_sbmnist.sh, run_vae_dbmnist.sh:28
    assert cfg.beta_schedule() == (1e-4, 1.0, 50000)
    assert net.TrainConfig(beta=0.5, beta_init=2.0, beta_annealing=7).beta_schedule() == (2.0, 0.5, 7)
    with pytest.raises(ValueError):
        net.TrainConfig(beta_annealing=6)                                          # a schedule needs its start
    with pytest.raises(ValueError):
        net.TrainConfig(beta_init=0.1, beta_annealing=2.5)


def test_schedule_values_follow_annealing_func():
    init, fin, ann = net.TrainConfig(beta=1.0, beta_init=0.1, beta_annealing=3).beta_schedule()
    assert [net.annealing_func(init, fin, ann, i) for i in (0, 3, 9)] == [0.1, 0.1 + 0.9 / 3.0 * 3.0, 0.1 + 0.9 / 3.0 * 3.0]
    assert net.annealing_func(0.1, 1.0, None, 5) == 1.0


DESC = ctypes.POINTER(L.ModelDesc)
NEW_ENTRY_POINTS = {
    "ardae_train_state_advance": [("state", vp), ("rng_inc", u64), ("lr", f64), ("beta1", f64), ("beta2", f64), ("beta_init", f64),
                                  ("beta_fin", f64), ("beta_annealing", i64), ("std_scale", f64), ("seed_rows", i64), ("stream", vp)],
    "ardae_seed_scale_dev": [("g", vp), ("n", i64), ("state", vp), ("stream", vp)],
    "ardae_model_vae_forward_dev": [("d", DESC), ("params", vp), ("packed", vp), ("x", vp), ("noise", vp), ("B", i32), ("nz", i32), ("state", vp),
                                    ("workspace", vp), ("workspace_floats", usize), ("z_out", vp), ("losses", vp), ("stream", vp)],
    "ardae_model_vae_backward_dev": [("d", DESC), ("params", vp), ("packed", vp), ("x", vp), ("noise", vp), ("B", i32), ("nz", i32), ("state", vp),
                                     ("dloss", f32), ("dz_extra", vp), ("workspace", vp), ("workspace_floats", usize), ("grads", vp),
                                     ("grads_beta", f32), ("stream", vp)],
    "ardae_model_vae_backward_decoder_dev": [("d", DESC), ("params", vp), ("packed", vp), ("x", vp), ("noise", vp), ("B", i32), ("nz", i32),
                                             ("state", vp), ("dloss", f32), ("workspace", vp), ("workspace_floats", usize), ("stream", vp)],
    "ardae_model_vae_backward_sampler_dev": [("d", DESC), ("params", vp), ("packed", vp), ("x", vp), ("noise", vp), ("B", i32), ("nz", i32),
                                             ("dz_extra", vp), ("state", vp), ("workspace", vp), ("workspace_floats", usize), ("grads", vp),
                                             ("grads_beta", f32), ("stream", vp)],
    "ardae_log_scalars_dev": [("cdae_loss", vp), ("model_losses", vp), ("std_b", vp), ("B", i32), ("beta_state", vp), ("d_lr", f32), ("state", vp),
                              ("ring", vp), ("capacity", i32), ("stream", vp)],
}
TWINS = {"ardae_model_vae_forward": "beta", "ardae_model_vae_backward": "beta", "ardae_model_vae_backward_decoder": "beta",
         "ardae_model_vae_backward_sampler": "seed_scale", "ardae_log_scalars": "beta"}


@pytest.mark.parametrize("name", sorted(NEW_ENTRY_POINTS))
def test_header_binds_the_new_entry_points(name):
    params = NEW_ENTRY_POINTS[name]
    assert L.EXPORTS[name] == (i32, [t for _, t in params])
    assert [p[0] for p in L.PROTOTYPES[name][1]] == [n for n, _ in params]


@pytest.mark.parametrize("name", sorted(TWINS))
def test_dev_twin_takes_the_block_where_the_value_form_takes_the_float(name):
    """The ardae_adam_ref_step / _dev precedent: the same parameter list, a `const void*` block in the float's place."""
    value, twin = L.PROTOTYPES[name][1], L.PROTOTYPES[name + "_dev"][1]
    assert len(value) == len(twin)
    k = [p[0] for p in value].index(TWINS[name])
    assert value[k][1:] == (f32, None) and twin[k][1:] == (vp, "void")
    assert [p for i, p in enumerate(value) if i != k] == [p for i, p in enumerate(twin) if i != k]


def test_abi_version_is_unchanged_and_the_library_exports_the_twins():
    assert L.CONSTANTS["ARDAE_ABI_VERSION"] == 1 and L.CONSTANTS["ARDAE_STEP_STATE_BYTES"] == 32
    if os.path.exists(L.LIB_PATH):          # (a tree without a built library: the header's side alone)
        h = L.lib()
        assert h.ardae_abi_version() == 1
        for name, params in NEW_ENTRY_POINTS.items():
            assert list(getattr(h, name).argtypes) == [t for _, t in params]
