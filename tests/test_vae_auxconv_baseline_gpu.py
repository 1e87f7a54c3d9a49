"""The hierarchical conv Gaussian baseline on the device (ardae_model_desc.kind 17; vae.py --model auxconv): forward / backward against the reference's
fixtures through the C ABI and through autograd on NaN-filled buffers with guard rows, the in-kernel draws, the recipe's widths against the float64
restatement of tests/test_vae_auxconv_baseline.py, the engine's trajectory, replay == eager, resume, the three-stage IWAE evaluation on fixed groups,
the drop-in route, and the decoder's last two stages as one kernel (ardae_conv_tail) against that restatement and the unfused launches.

The bodies these tests share with the other Gaussian families, and the tolerances, are tests/vae_gpu_checks.py's."""
import os
import subprocess
import sys

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
import vae_gpu_checks as G
import vae_restate as RS
from vae_gpu_checks import DEV, NAN, TOL_LATENT, TOL_MEAN, check_guard, guarded, load, rel
from test_vae_auxconv_baseline import CASES, D, auxconv_params, logprob_rows, logq_rows, loss_and_grads, restate, shape_of, tail_logit

pytestmark = pytest.mark.gpu
KNOB_ENV = {"ARDAE_DEBUG_KNOBS": "1", "ARDAE_CONV_TAIL_UNFUSED": "1"}
KNOB_ON = all(os.environ.get(k) == v for k, v in KNOB_ENV.items())      # (the child process of the last test)
ALL_ACTS = ("relu", "softplus", "elu", "tanh", "leaky_relu", "swish")


def build(nd, z, act, sd=None, **kw):
    m = net.MNISTConvAuxVAE(z0_dim=nd, z_dim=z, nonlinearity=act, **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    (B, nd, z), act = shape_of(fx)
    return build(nd, z, act, auxconv_params(fx))


def seeded(nd, z, act, seed):
    """A model with torch's default initialisation (non-zero biases everywhere) from a seed"""
    torch.manual_seed(seed)
    return build(nd, z, act, do_xavier=False)


# the z head's fused form (kind 11's tail form) is the default at z <= 64
FAMILY = G.Family(from_fixture=from_fixture, restate=restate, loss_and_grads=loss_and_grads, logprob_rows=logprob_rows, aux=True, image=True,
                  fixture_grads="norm", grads64=True, traj="ps", head_fused=1)


# ---- 1. both fixtures, both betas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    G.forward_backward_against_the_reference(FAMILY, golden_dir, "vae_" + case, f"auxconv {case}")


# ---- 2. the in-kernel draws ----------------------------------------------------------------------------------------------------------
def test_eps_null_draws_the_documented_philox_elements():
    B, nd, zd = 7, 5, 3                                    # B nd = 35: the second draw starts at element 36
    m = seeded(nd, zd, "softplus", 1)
    x = torch.bernoulli(torch.full((B, D), 0.3)).to(DEV)
    G.eps_null_draws_the_documented_philox_elements(m, x)


# ---- 3. the recipe's widths against the live float64 restatement ---------------------------------------------------------------------
def test_recipe_width_against_the_float64_restatement():
    B, nd, z, act = 70, 100, 32, "softplus"
    m = seeded(nd, z, act, 17)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, nd + z)
    G.against_the_float64_restatement(FAMILY, m, act, x, eps, [(beta, f"auxconv recipe width beta {beta}") for beta in (1.0, 0.3)])


# ---- 4. the engine's trajectory, replay == eager, resume ----------------------------------------------------------------------------
def test_engine_trajectory_against_the_reference(golden_dir):
    G.engine_trajectory_against_the_reference(FAMILY, golden_dir, "vae_traj_auxconv", "auxconv", steps=4)


def test_replay_equals_eager_and_resume_continues_to_the_same_bits():
    """One optimiser with a weight average: the captured step replays through the beta ramp, the checkpoint carries the average"""
    nd, z, B = 10, 6, 10
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(nd, z, "elu").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer="adam", lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg="polyak", weight_avg_start=1)
    a, _, _ = G.replay_equals_eager_and_resume(lambda: build(nd, z, "elu", sd0), xs, cfg, resume_at=3)
    # the step's draws are the documented elements at Philox offset RNG_STRIDE * step (+ 0), read through the state block
    assert torch.equal(a.eps, G.aux_draws(B, nd, z, 99, a.RNG_STRIDE * a.step_count))


# ---- 5. IWAE evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    G.iwae_on_injected_draws(FAMILY, golden_dir, "vae_" + case, case)


@pytest.mark.parametrize("B,k", [(3, 16), (5, 4)])
def test_aux_iwae_draw_against_float64_with_guard_rows(B, k):
    nd, zd, act = 11, 6, "elu"
    m = seeded(nd, zd, act, B * k)
    x = torch.bernoulli(torch.full((B, D), 0.3))
    eps = torch.randn(B, k, nd + zd)
    z, logq = G.aux_iwae_draw(m, x, eps)
    zw, lw = logq_rows(FAMILY.p64_of(m), act, x.double(), eps.double())
    assert rel(z.cpu(), zw) <= TOL_LATENT
    print(f"aux_iwae_draw kind 17 B={B} k={k}: logq rel L2 {rel(logq.cpu(), lw):.3g}")
    assert rel(logq.cpu(), lw) <= TOL_MEAN


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    """136 images at k = 4: one chunk against chunks of 64.  Every call runs on fixed groups (64 images for the statistics and the ELBO pass, 32 for
    the stages and the decoder), so elbo and logprob are equal to the bit."""
    N, k, nd, zd = 136, 4, 10, 6
    m = seeded(nd, zd, "softplus", 8)
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    G.iwae_does_not_depend_on_the_chunking(FAMILY, m, x, k, [(None, [136]), (100, [64, 64, 8])])


def test_iwae_runs_under_the_averaged_weights_and_puts_the_trained_ones_back():
    G.iwae_under_the_averaged_weights(seeded(10, 6, "softplus", 9), lambda: build(10, 6, "softplus"), B=8, lr=1e-3)


def test_drop_in_route_equals_the_engine(golden_dir):
    G.drop_in_route_equals_the_engine(FAMILY, golden_dir, "vae_traj_auxconv")


# ---- 6. the decoder's last two stages in one launch ----------------------------------------------------------------------------------
R_MAX = 70
# The bound on the fused kernel (variant 1) is measured against the existing path: the unfused launches' own relative L2 error to float64 on the
# same inputs, times 2 for the different summation order, floored at the fp32 level the residual-conv tail's test uses (TOL_LATENT = 1e-5).
# Measured on one MI355X (printed by the test below): see the docstring of test_tail_kernel_against_float64_and_the_unfused_launches.


def padded_u1(R, seed):
    """u1 [R, 8, 8, 32] from N(0, 1) with the pad positions (row 7, column 7) zeroed, as conv_decode_fwd leaves them"""
    u1 = torch.randn(R, 8, 8, 32, generator=torch.Generator().manual_seed(seed))
    u1[:, 7, :, :] = 0.0
    u1[:, :, 7, :] = 0.0
    return u1.contiguous()


@pytest.fixture(scope="module")
def tail_case(golden_dir):
    """The softplus fixture's decoder weights, one u1 [70, 8, 8, 32] and its float64 logits, shared by the tests below and left unchanged"""
    fx = load(golden_dir, "vae_" + CASES[0])
    m, (p64, act) = from_fixture(fx), restate(fx)
    u1 = padded_u1(R_MAX, 7502)
    return m, act, u1.to(DEV), tail_logit(p64, act, u1.double())


def tail(m, u1, variant):
    """-> logits [R, 784] of ardae_conv_tail on NaN-filled buffers, guard rows checked behind the logits and the workspace"""
    return G.abi_stage("ardae_conv_tail", m, u1, variant, D, "tail logits", expect_ws=variant == 2 or (variant == 0 and KNOB_ON))


def check_tail(m, u1, want, what):
    fused, unfused = tail(m, u1, 1), tail(m, u1, 2)
    e1, e2 = rel(fused.cpu(), want), rel(unfused.cpu(), want)
    bound = max(2.0 * e2, TOL_LATENT)
    print(f"tail {what}: fused against float64 rel L2 {e1:.3g}, unfused {e2:.3g}, bound {bound:.3g}; fused against unfused {rel(fused.cpu(), unfused.cpu()):.3g}")
    assert e2 <= TOL_LATENT and e1 <= bound
    return fused, unfused


@pytest.mark.parametrize("R", [1, 5, R_MAX])
def test_tail_kernel_against_float64_and_the_unfused_launches(tail_case, R):
    """conv_tail_kernel (variant 1) and the four unfused launches (variant 2) against the float64 restatement of stages A and B.  Measured on one
    MI355X at R = 70: fused 1.99e-7, unfused 1.21e-7 relative L2 to float64, so the bound is its floor, 1e-5 (2 x 1.21e-7 lies below it); under the
    other activations at R = 3 the fused kernel measured 1.6e-7 .. 3.4e-7, the unfused launches 0.8e-7 .. 1.5e-7.  The kernel is the library's
    choice (variant 0): 0.375 ms against 1.359 ms at the evaluator's 8192 rows (profiles/vae_auxconv_baseline_timing.json)."""
    m, act, u1, want = tail_case
    fused, unfused = check_tail(m, u1[:R].contiguous(), want[:R], f"R={R} {act}")
    default = 1 if L.query("ardae_conv_tail_workspace_floats", m._desc, R, 0) == 0 else 2
    assert default == 1                                                      # the library's choice is the kernel (README: the measurement)
    assert torch.equal(tail(m, u1[:R].contiguous(), 0), fused if default == 1 else unfused)


@pytest.mark.parametrize("act", ALL_ACTS)
def test_tail_kernel_under_every_activation(act):
    m = seeded(10, 6, act, 7600)
    u1 = padded_u1(3, 7601)
    check_tail(m, u1.to(DEV), tail_logit(FAMILY.p64_of(m), act, u1.double()), f"R=3 {act}")


def test_tail_kernel_rows_do_not_depend_on_the_rows_of_the_call(tail_case):
    m, _, u1, _ = tail_case
    assert torch.equal(tail(m, u1, 1)[:5], tail(m, u1[:5].contiguous(), 1))


def decode(m, z):
    """-> logits [R, 784] of ardae_model_decode and the u1 [R, 8, 8, 32] it left in its workspace (the decode-only carve opens with d1 [R, 300],
    d2 [R, 512], g0 [R, 512], c1 [R, 16, 800], u1, each rounded up to 64 floats)"""
    R = z.size(0)
    out, ws = G.abi_decode(m, z)
    al = lambda n: (n + 63) // 64 * 64      # noqa: E731
    off = al(R * 300) + 2 * al(R * 512) + al(R * 12800)
    return out, ws[off:off + R * 2048].view(R, 8, 8, 32).clone()


def other_kinds():
    """One small model of each kind that shares the conv decoder"""
    torch.manual_seed(7700)
    return {2: net.ConvIPVAE(z_dim=6, noise_dim=4).to(DEV), 4: net.MNISTConvAuxIPVAE(z0_dim=4, z_dim=6).to(DEV), 11: net.MNISTConvVAE(z_dim=6).to(DEV)}


def test_decode_only_path_and_the_other_kinds(tmp_path):
    """ardae_model_decode of kind 17 equals the u1 -> tail route, to the bit, and float64.  Under ARDAE_CONV_TAIL_UNFUSED=1 (a child process of the
    next test) it runs the unfused launches - it equals variant 2, its workspace grows - while kinds 2, 4 and 11 give the bits the parent left in a
    file: the new path does not leak into them."""
    unfused = KNOB_ON
    R = 11
    m = seeded(10, 6, "elu", 7701)
    z = torch.randn(R, 6, generator=torch.Generator().manual_seed(7702))
    logit, u1 = decode(m, z.to(DEV))
    assert bool(torch.isfinite(u1).all()) and float(u1[:, 7].abs().max()) == 0.0 and float(u1[:, :, 7].abs().max()) == 0.0
    assert torch.equal(logit, tail(m, u1, 2 if unfused else 1)) and torch.equal(logit, tail(m, u1, 0))
    assert (L.query("ardae_conv_tail_workspace_floats", m._desc, R, 0) > 0) == unfused
    assert (L.query("ardae_model_workspace_floats", m._desc, 1024, 1, 2) > L.query("ardae_conv_tail_workspace_floats", m._desc, 1024, 2)) == unfused
    assert rel(logit.cpu(), RS.conv_decode_logit(FAMILY.p64_of(m), "elu", z.double())) <= TOL_LATENT
    assert torch.equal(m.decode_params(z.to(DEV))[0], logit)
    u = torch.rand(R, D, generator=torch.Generator().manual_seed(7703))
    xs, mean, zz = m.generate(R, z=z.to(DEV), dec_noise=u.to(DEV))
    assert torch.equal(zz.cpu(), z) and torch.equal(mean, torch.sigmoid(logit)) and rel(xs.cpu(), RS.relaxed_sample(logit.double().cpu(), u.double())) <= 1e-4
    others = {}
    for kind, mod in other_kinds().items():
        wsf = L.query("ardae_model_workspace_floats", mod._desc, R, 1, 2)
        ws, out = torch.full((wsf,), NAN, device=DEV), guarded(R, D)
        L.call("ardae_model_decode", mod._desc, mod._flat, mod._packed_weights(), z.to(DEV), R, ws, wsf, out, None)
        check_guard(out, R, f"kind {kind} decode")
        others[kind] = out[:R].cpu()
    path = os.environ.get("AUXCONV_PARENT_OUTPUTS")
    if unfused:
        assert path, "the child process compares against the parent's outputs"
        parent = torch.load(path)
        for kind, out in others.items():
            assert torch.equal(out, parent[kind]), f"kind {kind}: ardae_model_decode changed under the knob"
        assert torch.equal(logit.cpu(), parent["variant2"])
        print("decode-only path, unfused launches: kind 17 equals variant 2; kinds 2, 4 and 11 unchanged")
    else:
        others["variant2"] = tail(m, u1, 2).cpu()
        torch.save(others, tmp_path / "parent.pt")


def test_decode_only_path_with_the_unfused_knob(tmp_path):
    """The library reads its debug knobs once per process, so the test above is re-run in a child process with the knob set."""
    test_decode_only_path_and_the_other_kinds(tmp_path)
    env = dict(os.environ, AUXCONV_PARENT_OUTPUTS=str(tmp_path / "parent.pt"), **KNOB_ENV)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "decode_only_path_and_the_other_kinds"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "kinds 2, 4 and 11 unchanged" in r.stdout, r.stdout[-500:]
