"""Gaussian-posterior VAE baselines on the device (ardae_model_desc.kind 8 / 9; vae.py --model mnist / toy): forward / backward against the
reference's fixtures through the C ABI and through autograd, the fused Gaussian head against the unfused launches, recipe widths against
the float64 restatement of tests/test_vae_baseline.py, the engine's trajectory, replay == eager, resume, IWAE evaluation, the drop-in route.

The bodies these tests share with the other Gaussian families, and the tolerances, are tests/vae_gpu_checks.py's."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import rng
import vae_gpu_checks as G
from vae_gpu_checks import DEV, TOL_MEAN, head, rel
from test_vae_baseline import case_names, logprob_rows, loss_and_grads, restate, state_dict_of

pytestmark = pytest.mark.gpu


def build(family, D, h, z, nl, act, sd=None):
    ctor = net.MNISTVAE if family == "mnist" else net.ToyVAE
    m = ctor(input_dim=D, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=nl)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    B, D, h, z, nl = (int(v) for v in fx["shape"])
    return build(str(fx["family"]), D, h, z, nl, str(fx["act"]), state_dict_of(fx))


FAMILY = G.Family(from_fixture=from_fixture, restate=restate, loss_and_grads=loss_and_grads, logprob_rows=logprob_rows, traj="p")


# ---- 5. forward / backward against the reference's fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("family,case", case_names())
def test_forward_backward_against_the_reference(golden_dir, family, case):
    G.forward_backward_against_the_reference(FAMILY, golden_dir, f"vae_{family}_{case}", f"{family} {case}")


def test_generate_and_the_in_kernel_draw_of_the_module():
    m = build("mnist", 20, 24, 4, 2, "softplus")
    net.manual_seed(5)
    xs, mean, z = m.generate(7)
    assert xs.shape == mean.shape == (7, 20) and z.shape == (7, 4) and bool(torch.isfinite(xs).all())
    x = torch.bernoulli(torch.full((9, 20), 0.3)).to(DEV)
    net.manual_seed(5)
    _, _, z1, loss1, _, _ = m(x)
    want = G.philox_normal((9, 4), 5, rng.HOST_STREAM | 0)
    _, _, z2, loss2, _, _ = m(x, eps=want)
    assert torch.equal(z1, z2) and torch.equal(loss1.detach(), loss2.detach())      # the head drew exactly that draw


# ---- 6. the fused head against the unfused launches --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,h,z", [(6, 40, 6), (70, 300, 32), (129, 256, 2)])
def test_fused_head_equals_the_unfused_launches(B, h, z):
    torch.manual_seed(B)
    family = "toy" if z == 2 else "mnist"
    m = build(family, 2 if z == 2 else 36, h, z, 2, "softplus")
    # the default is the fused kernel where both matrices' rows start on 16 bytes (the recipe's 300 -> 2 x 32), the unfused launches elsewhere
    assert L.query("ardae_vae_head_fused_ok", m._desc) == (1 if (h, z) == (300, 32) else 0)
    hid = torch.nn.functional.softplus(torch.randn(B, h)).to(DEV).contiguous()
    fused, unfused = head(m, hid, 1), head(m, hid, 2)
    draw = G.philox_normal((B, z), 123, 5)
    assert torch.equal(fused["eps"], draw) and torch.equal(unfused["eps"], draw)
    for k in ("mu", "lv", "z", "kld"):
        e = rel(fused[k].cpu(), unfused[k].cpu())
        same = float((fused[k] == unfused[k]).float().mean())
        print(f"head B={B} h={h} z={z} {k}: rel L2 {e:.3g}, bit-identical {100 * same:.1f} %")
        assert bool(torch.isfinite(fused[k]).all()) and e <= 1e-6
    # against float64 on the host
    G.check_head64(fused, *G.head64(m, hid), draw, "fused")
    # the variant the library picks, and an injected eps goes through unchanged
    auto, picked = head(m, hid, 0, eps=draw), (fused if L.query("ardae_vae_head_fused_ok", m._desc) else unfused)
    assert all(torch.equal(auto[k], picked[k]) for k in G.HEAD_KEYS)
    if B == 70:      # a row's bits do not depend on B
        small = head(m, hid[:6].contiguous(), 1)
        for k in G.HEAD_KEYS:
            assert torch.equal(small[k], fused[k][:6]), k


# ---- 7. recipe width against the live float64 restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("family,D,h,z,act,B", [("mnist", 784, 300, 32, "softplus", 70), ("toy", 2, 256, 2, "relu", 129)])
def test_recipe_width_against_the_float64_restatement(family, D, h, z, act, B):
    torch.manual_seed(17)
    m = build(family, D, h, z, 2, act)
    x = (torch.bernoulli(torch.full((B, D), 0.3)) if family == "mnist" else torch.randn(B, D))
    eps = torch.randn(B, z)
    G.against_the_float64_restatement(FAMILY, m, (family, act), x, eps, [(beta, f"{family} recipe width beta {beta}") for beta in (1.0, 0.3)])


# ---- 8. the engine's trajectory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["mnist", "toy"])
def test_engine_trajectory_against_the_reference(golden_dir, family):
    G.engine_trajectory_against_the_reference(FAMILY, golden_dir, f"vae_traj_{family}", family, steps=5)


# ---- 9. replay == eager, resume -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,optimizer,avg", [("mnist", "adam", "swa"), ("toy", "rmsprop", "none"), ("mnist", "amsgrad", "polyak")])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(family, optimizer, avg):
    D, h, z, B = (36, 48, 8, 10) if family == "mnist" else (2, 40, 2, 12)
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(family, D, h, z, 2, "softplus").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [(torch.bernoulli(torch.full((B, D), 0.3), generator=g) if family == "mnist" else torch.randn(B, D, generator=g)).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer=optimizer, lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)
    a, _, _ = G.replay_equals_eager_and_resume(lambda: build(family, D, h, z, 2, "softplus", sd0), xs, cfg, resume_at=3)
    # the step's own draw is the separate draw at Philox offset RNG_STRIDE * step (+ 0), read through the state block
    assert a.RNG_STRIDE == 16 and torch.equal(a.eps, G.philox_normal((B, z), 99, a.RNG_STRIDE * a.step_count))


# ---- 10. IWAE evaluation under the analytic posterior -------------------------------------------------------------------------------
@pytest.mark.parametrize("family,case", case_names())
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, family, case):
    fx, m, x = G.iwae_on_injected_draws(FAMILY, golden_dir, f"vae_{family}_{case}", f"{family} {case}")
    # the KL rows the evaluator reduces are the head's
    mu, lv = m.encode_stats(x)
    rows_kld = torch.empty(x.size(0), device=DEV)
    L.call("ardae_vae_kld_rows", mu, lv, x.size(0), m.z_dim, rows_kld)
    assert rel(rows_kld.cpu(), -0.5 * (1 + fx["lv_f64"] - fx["mu_f64"] ** 2 - np.exp(fx["lv_f64"])).sum(1)) <= TOL_MEAN


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    torch.manual_seed(8)
    m = build("mnist", 36, 48, 8, 2, "softplus")
    x = torch.bernoulli(torch.full((12, 36), 0.3)).to(DEV)
    G.iwae_does_not_depend_on_the_chunking(FAMILY, m, x, 16, [(12, 1), (8, 2), (4, 3)])


def test_iwae_runs_under_the_averaged_weights_and_puts_the_trained_ones_back():
    torch.manual_seed(9)
    G.iwae_under_the_averaged_weights(build("mnist", 36, 48, 8, 2, "softplus"), lambda: build("mnist", 36, 48, 8, 2, "softplus"), B=8, lr=1e-2)


# ---- 11. the drop-in route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["mnist", "toy"])
def test_drop_in_route_equals_the_engine(golden_dir, family):
    G.drop_in_route_equals_the_engine(FAMILY, golden_dir, f"vae_traj_{family}")
