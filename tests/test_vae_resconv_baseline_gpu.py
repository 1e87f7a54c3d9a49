"""The residual-conv Gaussian-posterior baseline on the device (ardae_model_desc.kind 12; vae.py --model resconv): forward / backward against the
reference's fixtures through the C ABI and through autograd, shapes the fixtures do not reach against the float64 restatement of
tests/test_vae_resconv_baseline.py with NaN-filled buffers and guard rows, the decoder's last stage as one kernel (ardae_resconv_tail) against that
restatement and against the unfused launches, the decode-only path, the Gaussian head at c_dim 450 / 42, the engine's trajectory, replay == eager,
resume, IWAE evaluation.

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
from vae_gpu_checks import DEV, TOL_LATENT, head, rel
from test_vae_resconv_baseline import CASES, D, fixture_params, logprob_rows, loss_and_grads, resconv_params, restate, trajectory

pytestmark = pytest.mark.gpu
KNOB_ENV = {"ARDAE_DEBUG_KNOBS": "1", "ARDAE_RESCONV_TAIL_UNFUSED": "1"}


def build(z, c_dim, center=False, sd=None, **kw):
    m = net.MNISTResConvVAE(z_dim=z, c_dim=c_dim, do_center=center, **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def seeded(z, c_dim, center, seed):
    """a module on the oracle's initialiser: weight-norm scales spread over [0.7, 1.3], not torch's 1"""
    return build(z, c_dim, center, resconv_params(z, c_dim, seed, False))


def from_fixture(fx):
    B, z, c = (int(v) for v in fx["shape"])
    return build(z, c, bool(int(fx["do_center"])), fixture_params(fx))


FAMILY = G.Family(from_fixture=from_fixture, restate=restate, loss_and_grads=loss_and_grads, logprob_rows=logprob_rows, image=True, fixture_grads="norm",
                  grads64=True, traj="restate", trajectory=trajectory, logprob_is_evaluator=True)


# ---- 1. both fixtures, both betas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    G.forward_backward_against_the_reference(FAMILY, golden_dir, f"vae_resconv_{case}", f"resconv {case}")


# ---- 2. shapes the fixtures do not reach, against the float64 restatement ----------------------------------------------------------
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("B", [1, 9, 70])
def test_other_batches_against_the_float64_restatement_with_guard_rows(B, center):
    """B = 1; one row past the head's 8-row tile; past a 64-row tile.  do_center on runs the narrow model (c_dim 42, z 6: head rows off the 16-byte
    grid), off the recipe's widths.  Every buffer starts as NaN, so a read of something never written shows in the results, and nothing past B rows
    of any caller buffer (or past the workspace's declared size) may be written."""
    z, c = (6, 42) if center else (32, 450)
    torch.manual_seed(100 + B)
    m = seeded(z, c, center, 7000 + B)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, z)
    out, zc = G.against_the_float64_restatement(FAMILY, m, center, x, eps, [(0.3, f"resconv B={B} center={center}")])
    # encode_stats and decode: the same guards
    mu, lv = G.abi_encode_stats(m, x.to(DEV), z)
    assert rel(mu.cpu(), out["mu"]) <= TOL_LATENT and rel(lv.cpu(), out["lv"]) <= TOL_LATENT
    logit, _ = G.abi_decode(m, zc)
    assert rel(logit.cpu(), out["logit"]) <= TOL_LATENT


# ---- 3. the decoder's last stage in one launch ---------------------------------------------------------------------------------------
R_MAX = 67


@pytest.fixture(scope="module")
def tail_case():
    """One model (randomly initialised, non-unit scales), one y14 [67, 14, 14, 16] with values above -1 as ELU outputs are - different at every
    pixel and channel - and its float64 logits, shared by the tests below and left unchanged."""
    m = seeded(6, 42, False, 7301)
    g = torch.Generator().manual_seed(7302)
    y = torch.nn.functional.elu(1.5 * torch.randn(R_MAX, 14, 14, 16, generator=g)).contiguous()
    assert float(y.min()) > -1.0
    want = RS.resconv_tail_logit(FAMILY.p64_of(m), y.double())
    return m, y.to(DEV), want


def tail(m, y, variant):
    """-> logits [R, 784] of ardae_resconv_tail on NaN-filled buffers, guard rows checked behind the logits and the workspace"""
    return G.abi_stage("ardae_resconv_tail", m, y, variant, D, "tail logits", expect_ws=variant == 2)


def border_mask():
    b = torch.zeros(28, 28, dtype=torch.bool)
    b[0, :] = b[27, :] = b[:, 0] = b[:, 27] = True
    return b.reshape(D)


@pytest.mark.parametrize("R", [1, 3, R_MAX])
def test_tail_kernel_against_float64_and_the_unfused_launches(tail_case, R):
    """Variant 1 against the float64 restatement (F.interpolate(align_corners=True), then O.res_conv of decode.dec.17) and against variant 2, over
    all pixels and over the border pixels alone: the padding taps at the four edges, and output index 27, where the source index lands on 13."""
    m, y, want = tail_case
    yr, wr = y[:R].contiguous(), want[:R]
    fused, unfused = tail(m, yr, 1), tail(m, yr, 2)
    edge = border_mask()
    for name, got in (("fused", fused), ("unfused", unfused)):
        e_all, e_edge = rel(got.cpu(), wr), rel(got.cpu()[:, edge], wr[:, edge])
        print(f"tail R={R} {name} against float64: rel L2 {e_all:.3g}, border pixels {e_edge:.3g}")
        assert e_all <= TOL_LATENT and e_edge <= TOL_LATENT
    e_all, e_edge = rel(fused.cpu(), unfused.cpu()), rel(fused.cpu()[:, edge], unfused.cpu()[:, edge])
    print(f"tail R={R} fused against unfused: rel L2 {e_all:.3g}, border pixels {e_edge:.3g}, bit-identical {100 * float((fused == unfused).float().mean()):.1f} %")
    assert e_all <= TOL_LATENT and e_edge <= TOL_LATENT
    assert torch.equal(tail(m, yr, 0), fused)                  # the library's choice is the kernel (README)


def test_tail_kernel_rows_do_not_depend_on_the_rows_of_the_call(tail_case):
    m, y, _ = tail_case
    full = tail(m, y, 1)
    for r in (0, R_MAX - 1):
        assert torch.equal(tail(m, y[r:r + 1].contiguous(), 1)[0], full[r]), r


# ---- 4. the decode-only path ---------------------------------------------------------------------------------------------------------
def test_decode_only_path_against_the_restatement(tmp_path):
    """decode_params and generate (injected z and dec_noise) against float64.  Under ARDAE_RESCONV_TAIL_UNFUSED=1 (a child process of the next
    test) the path runs the unfused launches, its workspace grows, and the logits equal the kernel's, which the parent left in a file."""
    unfused = all(os.environ.get(k) == v for k, v in KNOB_ENV.items())
    m = seeded(6, 42, False, 7401)
    R = 11
    g = torch.Generator().manual_seed(7402)
    z, u = torch.randn(R, 6, generator=g), torch.rand(R, D, generator=g)
    want = RS.resconv_decode_logit(FAMILY.p64_of(m), z.double())
    assert (L.query("ardae_resconv_tail_workspace_floats", m._desc, R, 0) > 0) == unfused
    # the last stage's own buffers (u28, dec[6]'s columns) outweigh everything the kernel's path keeps
    assert (L.query("ardae_model_workspace_floats", m._desc, 2048, 1, 2) > L.query("ardae_resconv_tail_workspace_floats", m._desc, 2048, 2)) == unfused
    logit = m.decode_params(z.to(DEV))[0]
    assert logit.shape == (R, D) and rel(logit.cpu(), want) <= TOL_LATENT
    xs, mean, zz = m.generate(R, z=z.to(DEV), dec_noise=u.to(DEV))
    assert torch.equal(zz.cpu(), z) and rel(mean.cpu(), torch.sigmoid(want)) <= TOL_LATENT
    assert rel(xs.cpu(), RS.relaxed_sample(want, u.double())) <= 1e-4
    path = os.environ.get("RESCONV_FUSED_LOGITS")
    if unfused:
        assert path, "the child process compares against the parent's logits"
        e = rel(logit.cpu(), torch.load(path))
        print(f"decode-only path, unfused launches against the kernel: rel L2 {e:.3g}")
        assert e <= TOL_LATENT
    else:
        torch.save(logit.cpu(), tmp_path / "fused.pt")


def test_decode_only_path_with_the_unfused_knob(tmp_path):
    """The library reads its debug knobs once per process, so the test above is re-run in a child process with the knob set."""
    test_decode_only_path_against_the_restatement(tmp_path)
    env = dict(os.environ, RESCONV_FUSED_LOGITS=str(tmp_path / "fused.pt"), **KNOB_ENV)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "decode_only_path_against_the_restatement"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "unfused launches against the kernel" in r.stdout, r.stdout[-500:]


# ---- 5. the head at c_dim 450 and 42 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,z", [(450, 32), (42, 6)])
@pytest.mark.parametrize("B", [1, 70])
def test_head_variants_against_float64(B, c, z):
    """gauss_head_kernel (variant 1) and the unfused launches (variant 2) on c_dim-wide hidden rows, own draw and injected eps, against float64 on
    the host.  The default is what README says: the unfused launches (450 is no multiple of 4: the kernel reads float by float and loses)."""
    torch.manual_seed(B + c)
    m = seeded(z, c, False, 7500 + c)
    assert L.query("ardae_vae_head_fused_ok", m._desc) == 0
    hid = torch.nn.functional.elu(torch.randn(B, c)).to(DEV).contiguous()
    draw = G.philox_normal((B, z), 123, 5)
    given = torch.randn(B, z).to(DEV)
    mu, lv = G.head64(m, hid)
    for eps, used in ((None, draw), (given, given)):
        fused, unfused = head(m, hid, 1, eps), head(m, hid, 2, eps)
        assert torch.equal(fused["eps"], used) and torch.equal(unfused["eps"], used)
        for name, v in (("fused", fused), ("unfused", unfused)):
            G.check_head64(v, mu, lv, used, name)
        auto = head(m, hid, 0, eps)
        assert all(torch.equal(auto[k], unfused[k]) for k in G.HEAD_KEYS)


# ---- 6. the engine -------------------------------------------------------------------------------------------------------------------
def test_engine_trajectory_against_the_reference(golden_dir):
    G.engine_trajectory_against_the_reference(FAMILY, golden_dir, "vae_traj_resconv", "resconv", steps=4)


@pytest.mark.parametrize("avg", ["none", "polyak"])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(avg):
    B, z, c = 8, 8, 40
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(z, c).state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(lr=1e-3, beta1=0.9, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)
    G.replay_equals_eager_and_resume(lambda: build(z, c, sd=sd0), xs, cfg, resume_at=4)       # a fresh engine continues for 2 steps


# ---- 7. evaluate_iws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    G.iwae_on_injected_draws(FAMILY, golden_dir, f"vae_resconv_{case}", f"resconv {case}")


def test_iwae_does_not_depend_on_the_chunking():
    """One chunk of 200 images against chunks of 64 (three encoder groups and a tail of 8) at k = 4: the evaluator calls the encoder and the ELBO
    pass's decoder on 64 images and the importance samples' decoder on 8 under either plan, so everything is equal to the bit."""
    torch.manual_seed(8)
    zd = 8
    m = build(zd, 40)
    N, k = 200, 4
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(N, k, zd).to(DEV), torch.randn(N, zd).to(DEV)
    assert m._eval_groups == (64, 8)
    # two budgets, two chunk lengths (whole groups under a budget of 100 images)
    G.iwae_does_not_depend_on_the_chunking(FAMILY, m, x, k, [(200, [200]), (100, [64, 64, 64, 8])], eps, fwd_eps)
