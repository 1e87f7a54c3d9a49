"""Auxiliary-variable Gaussian baselines on the device (ardae_model_desc.kind 14 / 15; vae.py --model auxmnist / auxtoy): forward / backward against
the reference's fixtures through the C ABI and through autograd, the pair-KL rows, the in-kernel draws, recipe widths against the float64 restatement
of tests/test_vae_aux_baseline.py, the engine's trajectory, replay == eager, resume, the three-stage IWAE evaluation, the drop-in route.

The bodies these tests share with the other Gaussian families, and the tolerances, are tests/vae_gpu_checks.py's."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
import vae_gpu_checks as G
from vae_gpu_checks import DEV, TOL_LATENT, TOL_MEAN, abi_forward_backward, check_losses, np64, rel
from vae_restate import aux_logq_rows, pair_kld_rows
from test_vae_aux_baseline import CASES, TRAJ, aux_params, forward_backward, logprob_rows, restate, shape_of

pytestmark = pytest.mark.gpu


def build(family, D, nd, h, z, nl, act, clip=None, sd=None):
    ctor = net.MNISTAuxVAE if family == "mnist" else net.ToyAuxVAE
    m = ctor(input_dim=D, noise_dim=nd, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=nl, clip_logvar=clip)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    family, (B, D, h, nd, z, nl), act, clip = shape_of(fx)
    return build(family, D, nd, h, z, nl, act, clip, aux_params(fx))


FAMILY = G.Family(from_fixture=from_fixture, restate=restate, loss_and_grads=forward_backward, logprob_rows=logprob_rows, to64=np64, aux=True)


# ---- 1. forward / backward against the reference's fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    G.forward_backward_against_the_reference(FAMILY, golden_dir, "vae_" + case, case)


# ---- 2. the pair KL -------------------------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(1, 1), (5, 10), (70, 100), (129, 128)]


def pair_inputs(B, n):
    g = torch.Generator().manual_seed(100 * B + n)
    return [(torch.randn(B, n, generator=g) * s).to(DEV).contiguous() for s in (1.0, 1.5, 1.0, 0.7)]      # mu1, lv1, mu2, lv2


@pytest.fixture(scope="module")
def pair_at_129():
    mu1, lv1, mu2, lv2 = pair_inputs(129, 128)
    out = torch.full((130,), float("nan"), device=DEV)
    L.call("ardae_vae_pair_kld_rows", mu1, lv1, mu2, lv2, 129, 128, out)
    return (mu1, lv1, mu2, lv2), out


@pytest.mark.parametrize("B,n", PAIR_SHAPES)
def test_pair_kld_rows_against_float64(B, n, pair_at_129):
    if (B, n) == (129, 128):
        (mu1, lv1, mu2, lv2), out = pair_at_129
    else:
        mu1, lv1, mu2, lv2 = pair_inputs(B, n)
        out = torch.full((B + 1,), float("nan"), device=DEV)
        L.call("ardae_vae_pair_kld_rows", mu1, lv1, mu2, lv2, B, n, out)
    want = pair_kld_rows(np64(mu1), np64(lv1), np64(mu2), np64(lv2))
    assert bool(torch.isnan(out[B])) and rel(np64(out[:B]), want) <= TOL_MEAN
    assert float(np.max(np.abs(np64(out[:B]) - want) / np.abs(want))) <= TOL_MEAN      # row by row, not only in the norm


def test_pair_kld_row_bits_do_not_depend_on_the_batch(pair_at_129):
    (mu1, lv1, mu2, lv2), out = pair_at_129
    for r0 in (0, 63, 126):
        small = torch.empty(3, device=DEV)
        L.call("ardae_vae_pair_kld_rows", *(t[r0:r0 + 3].contiguous() for t in (mu1, lv1, mu2, lv2)), 3, 128, small)
        assert torch.equal(small, out[r0:r0 + 3]), r0


@pytest.mark.parametrize("B,n", PAIR_SHAPES)
def test_the_forward_adds_the_pair_kld_into_the_heads_rows(B, n):
    """losses[2] = mean(kld + aux_kld): the head's KL rows (ardae_vae_kld_rows on the head's statistics) + ardae_vae_pair_kld_rows, in float64"""
    torch.manual_seed(B + n)
    m = build("toy", 2, n, 24, 3, 2, "tanh", "spm6")
    x, eps = torch.randn(B, 2), torch.randn(B, n + 3)
    out, _ = forward_backward(FAMILY.p64_of(m), ("toy", "tanh", "spm6"), np64(x), np64(eps), 1.0, 1.0)
    _, losses, _, _ = abi_forward_backward(m, x.to(DEV), eps.to(DEV), 1.0, 1.0)
    check_losses(losses.tolist(), out, f"pair KL in the forward B={B} n={n}")


# ---- 3. the in-kernel draws ----------------------------------------------------------------------------------------------------------
def test_eps_null_draws_the_documented_philox_elements():
    B, nd, zd = 7, 5, 3                                    # B nd = 35: the second draw starts at element 36
    torch.manual_seed(1)
    m = build("mnist", 20, nd, 24, zd, 2, "softplus", "hard")
    x = torch.bernoulli(torch.full((B, 20), 0.3)).to(DEV)
    G.eps_null_draws_the_documented_philox_elements(m, x)


# ---- 4. recipe widths against the live float64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,D,nd,h,z,nl,act,B", [("mnist", 784, 100, 300, 32, 2, "softplus", 70), ("toy", 2, 2, 64, 2, 1, "tanh", 129)])
def test_recipe_width_against_the_float64_restatement(family, D, nd, h, z, nl, act, B):
    torch.manual_seed(17)
    m = build(family, D, nd, h, z, nl, act)
    x = (torch.bernoulli(torch.full((B, D), 0.3)) if family == "mnist" else torch.randn(B, D))
    eps = torch.randn(B, nd + z)
    G.against_the_float64_restatement(FAMILY, m, (family, act, None), x, eps, [(beta, f"{family} recipe width beta {beta}") for beta in (1.0, 0.3)])


# ---- 5. the engine's trajectory, replay == eager, resume ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRAJ)
def test_engine_trajectory_against_the_reference(golden_dir, name):
    G.engine_trajectory_against_the_reference(FAMILY, golden_dir, "vae_traj_" + name, name, steps=4)


@pytest.mark.parametrize("family,optimizer,avg", [("mnist", "adam", "swa"), ("toy", "amsgrad", "polyak")])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(family, optimizer, avg):
    D, nd, h, z, B = (36, 10, 48, 8, 10) if family == "mnist" else (2, 5, 40, 3, 12)
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(family, D, nd, h, z, 2, "softplus", "spm4").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [(torch.bernoulli(torch.full((B, D), 0.3), generator=g) if family == "mnist" else torch.randn(B, D, generator=g)).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer=optimizer, lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)
    a, _, da = G.replay_equals_eager_and_resume(lambda: build(family, D, nd, h, z, 2, "softplus", "spm4", sd0), xs, cfg, resume_at=3)
    # the step's draws are the documented elements at Philox offset RNG_STRIDE * step (+ 0), read through the state block ...
    assert torch.equal(a.eps, G.aux_draws(B, nd, z, 99, a.RNG_STRIDE * a.step_count))
    # ... and two consecutive steps draw disjoint numbers
    for s in range(5):
        assert not bool(torch.isin(da[s].flatten(), da[s + 1].flatten()).any()), s


# ---- 6. IWAE evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    G.iwae_on_injected_draws(FAMILY, golden_dir, "vae_" + case, case)


@pytest.mark.parametrize("B,k", [(3, 16), (5, 4)])
def test_aux_iwae_draw_against_float64_with_guard_rows(B, k):
    torch.manual_seed(B * k)
    D, nd, zd = 20, 11, 6
    m = build("mnist", D, nd, 24, zd, 2, "elu", "2tanh")
    x = torch.bernoulli(torch.full((B, D), 0.3))
    eps = torch.randn(B, k, nd + zd)
    z, logq = G.aux_iwae_draw(m, x, eps)
    zw, lw = aux_logq_rows(FAMILY.p64_of(m), ("mnist", "elu", "2tanh"), np64(x), np64(eps))
    assert rel(np64(z), zw) <= TOL_LATENT
    print(f"aux_iwae_draw B={B} k={k}: logq rel L2 {rel(np64(logq), lw):.3g}")
    assert rel(np64(logq), lw) <= TOL_MEAN


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    torch.manual_seed(8)
    N, k, D, nd, zd = 40, 16, 36, 10, 8
    m = build("mnist", D, nd, 48, zd, 2, "softplus", "spm4")
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    G.iwae_does_not_depend_on_the_chunking(FAMILY, m, x, k, [(40, 1), (16, 3), (8, 5)])


def test_iwae_runs_under_the_averaged_weights_and_puts_the_trained_ones_back():
    torch.manual_seed(9)
    make = lambda: build("mnist", 36, 10, 48, 8, 2, "softplus")      # noqa: E731
    G.iwae_under_the_averaged_weights(make(), make, B=8, lr=1e-2)


# ---- 7. the drop-in route --------------------------------------------------------------------------------------------------------------
def test_drop_in_route_equals_the_engine(golden_dir):
    G.drop_in_route_equals_the_engine(FAMILY, golden_dir, "vae_traj_auxmnist")
