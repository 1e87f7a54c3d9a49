"""The hierarchical resconv Gaussian baseline on the device (ardae_model_desc.kind 19; vae.py --model auxresconv / auxresconvct): forward / backward
against the reference's fixtures through the C ABI and through autograd on NaN-filled buffers with guard rows, other batches against the float64
restatement of tests/test_vae_auxresconv_baseline.py, the decoder's 14 x 14 stage as one kernel (ardae_resconv_mid) against that restatement and the
unfused launches, the decode-only path with and without the knob, the engine's trajectory, replay == eager, resume, and the three-stage IWAE evaluation
on fixed groups.

The bodies these tests share with the other Gaussian families, and the tolerances, are tests/vae_gpu_checks.py's."""
import os
import subprocess
import sys

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
import vae_gpu_checks as G
from vae_gpu_checks import DEV, NAN, TOL_LATENT, check_guard, guarded, load, rel
from test_vae_auxresconv_baseline import CASES, D, auxres_params, decode_logit, head_map, logprob_rows, loss_and_grads, mid_map, restate, shape_of

pytestmark = pytest.mark.gpu
KNOB_ENV = {"ARDAE_DEBUG_KNOBS": "1", "ARDAE_RESCONV_MID_UNFUSED": "1"}
KNOB_ON = all(os.environ.get(k) == v for k, v in KNOB_ENV.items())      # (the child process of the last decode test)


def build(nd, z, c, center, sd=None):
    m = net.MNISTResConvAuxVAE(z0_dim=nd, z_dim=z, c_dim=c, do_center=center)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    (B, nd, z, c), center = shape_of(fx)
    return build(nd, z, c, center, auxres_params(fx))


def seeded(nd, z, c, center, seed):
    torch.manual_seed(seed)
    return build(nd, z, c, center)


# the z head has kind 12's policy: the unfused launches
FAMILY = G.Family(from_fixture=from_fixture, restate=restate, loss_and_grads=loss_and_grads, logprob_rows=logprob_rows, aux=True, image=True,
                  fixture_grads="norm", grads64=True, traj="ps", head_fused=0)


# ---- 1. both fixtures, both betas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    G.forward_backward_against_the_reference(FAMILY, golden_dir, "vae_" + case, f"auxresconv {case}")


# ---- 2. other batches against the live float64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,nd,z,c,center", [(1, 10, 6, 42, True), (9, 10, 6, 42, True), (65, 10, 6, 42, True), (9, 100, 32, 450, False)])
def test_other_batches_against_the_float64_restatement(B, nd, z, c, center):
    m = seeded(nd, z, c, center, 17 + B)
    g = torch.Generator().manual_seed(B)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3), generator=g), torch.randn(B, nd + z, generator=g)
    G.against_the_float64_restatement(FAMILY, m, center, x, eps, [(0.3, f"auxresconv B={B} c_dim {c}")])


# ---- 3. the decoder's 14 x 14 stage in one launch ------------------------------------------------------------------------------------
R_MAX = 5
MID_DEFAULT = 1      # the library's choice (README: the measurement at both call shapes)


@pytest.fixture(scope="module")
def mid_case(golden_dir):
    """The recipe fixture's decoder weights, one y8 [5, 8, 8, 32] whose cropped strip (row 7, column 7) is NaN, and the float64 y14 of the same numbers,
    shared by the tests below and left unchanged"""
    fx = load(golden_dir, "vae_" + CASES[0])
    m = from_fixture(fx)
    y8 = torch.randn(R_MAX, 8, 8, 32, generator=torch.Generator().manual_seed(7702))
    want = mid_map(restate(fx)[0], y8.double())
    y8[:, 7, :, :] = NAN
    y8[:, :, 7, :] = NAN
    return m, y8.contiguous().to(DEV), want


def mid(m, y8, variant):
    """-> y14 [R, 14, 14, 16] of ardae_resconv_mid on NaN-filled buffers, guard rows checked behind y14 and the workspace"""
    out = G.abi_stage("ardae_resconv_mid", m, y8, variant, 196 * 16, "mid y14", expect_ws=variant == 2 or (variant == 0 and KNOB_ON))
    return out.view(y8.size(0), 14, 14, 16)


def border(t):
    """the output positions whose source index lands on 0 or 6: index 0 and 13 in each direction"""
    return torch.cat([t[:, 0].reshape(-1), t[:, 13].reshape(-1), t[:, 1:13, 0].reshape(-1), t[:, 1:13, 13].reshape(-1)])


@pytest.mark.parametrize("R", [1, 3, R_MAX])
def test_mid_kernel_against_float64_and_the_unfused_launches(mid_case, R):
    """resconv_mid_kernel (variant 1) and the ten unfused launches (variant 2) against the float64 restatement of the stage, over all positions and over
    the border positions alone; y8's cropped strip is NaN, so any read of it shows.  Both are fp32 chains over the same 288 + 144 products per output;
    the kernel's relative L2 error may be at most twice the launches' on the same inputs (the factor covers the summation order).  The figures are
    printed; measured on one MI355X at R = 5: fused 5.76e-7, unfused 3.77e-7 over all positions (bound 7.54e-7), 5.12e-7 against 3.44e-7 on the border.
    The kernel is the library's choice (variant 0): 0.072 against 0.248 ms at 128 rows, 0.719 against 3.479 ms at the evaluator's 4096
    (profiles/vae_auxresconv_baseline_timing.json)."""
    m, y8, want = mid_case
    fused, unfused = mid(m, y8[:R].contiguous(), 1), mid(m, y8[:R].contiguous(), 2)
    for what, f in (("all positions", lambda t: t.reshape(-1)), ("border positions", border)):
        e1, e2 = rel(f(fused.cpu()), f(want[:R])), rel(f(unfused.cpu()), f(want[:R]))
        print(f"mid R={R} {what}: fused against float64 rel L2 {e1:.3g}, unfused {e2:.3g}, bound {2 * e2:.3g}; fused against unfused "
              f"{rel(f(fused.cpu()), f(unfused.cpu())):.3g}")
        assert e2 <= TOL_LATENT and e1 <= 2.0 * e2
    default = 1 if L.query("ardae_resconv_mid_workspace_floats", m._desc, R, 0) == 0 else 2
    assert default == (2 if KNOB_ON else MID_DEFAULT)
    assert torch.equal(mid(m, y8[:R].contiguous(), 0), fused if default == 1 else unfused)


def test_mid_kernel_rows_do_not_depend_on_the_rows_of_the_call(mid_case):
    m, y8, _ = mid_case
    whole = mid(m, y8, 1)
    for r in (0, 4):
        assert torch.equal(whole[r], mid(m, y8[r:r + 1].contiguous(), 1)[0])


def decode(m, z, unfused):
    """-> logits [R, 784] of ardae_model_decode and the y8 [R, 8, 8, 32] it left in its workspace (the decode-only carve opens with the two columns
    scratches, then hidden map and output of dec[0] .. dec[3], each rounded up to 64 floats)"""
    R = z.size(0)
    out, ws = G.abi_decode(m, z)
    al = lambda n: (n + 63) // 64 * 64      # noqa: E731
    cols = al(R * 196 * 288) + al(R * 196 * 144) if unfused else 2 * al(R * 64 * 288)
    off = cols + 2 * al(R * m.c_dim) + 2 * al(R * 512) + 3 * al(R * 2048)
    return out, ws[off:off + R * 2048].view(R, 8, 8, 32).clone()


def tail(m, y14):
    R = y14.size(0)
    out = guarded(R, D)
    L.call("ardae_resconv_tail", m._desc, m._flat, m._packed_weights(), y14.contiguous(), R, 1, None, 0, out)
    check_guard(out, R, "tail logits")
    return out[:R].clone()


def test_decode_only_path_and_kind_12(tmp_path):
    """ardae_model_decode of kind 19 equals dec[0 .. 3] -> ardae_resconv_mid -> ardae_resconv_tail, to the bit, and float64.  Under
    ARDAE_RESCONV_MID_UNFUSED=1 (a child process of the next test) it runs the unfused launches - it equals variant 2, its workspace grows - while
    kind 12 gives the bits the parent left in a file: the new path does not leak into it."""
    unfused = KNOB_ON
    R = 11
    m = seeded(10, 6, 42, True, 7701)
    z = torch.randn(R, 6, generator=torch.Generator().manual_seed(7702))
    logit, y8 = decode(m, z.to(DEV), unfused)
    assert bool(torch.isfinite(y8).all())
    assert rel(y8.cpu(), head_map(FAMILY.p64_of(m), z.double())) <= TOL_LATENT
    assert torch.equal(logit, tail(m, mid(m, y8, 2 if unfused else 1)))
    if not unfused and MID_DEFAULT == 1:
        assert torch.equal(logit, tail(m, mid(m, y8, 0)))
    assert (L.query("ardae_resconv_mid_workspace_floats", m._desc, R, 0) > 0) == (unfused or MID_DEFAULT == 2)
    assert rel(logit.cpu(), decode_logit(FAMILY.p64_of(m), z.double())) <= TOL_LATENT
    assert torch.equal(m.decode_params(z.to(DEV))[0], logit)
    torch.manual_seed(7700)
    m12 = net.MNISTResConvVAE(z_dim=6, c_dim=42).to(DEV)
    out, _ = G.abi_decode(m12, z.to(DEV), "kind 12 decode", slack=0)
    ws19 = L.query("ardae_model_workspace_floats", m._desc, 1024, 1, 2)
    path = os.environ.get("AUXRESCONV_PARENT_OUTPUTS")
    if unfused:
        assert path, "the child process compares against the parent's outputs"
        parent = torch.load(path)
        assert torch.equal(out.cpu(), parent["kind12"]), "kind 12: ardae_model_decode changed under the knob"
        assert torch.equal(logit.cpu(), parent["variant2"])
        assert ws19 > parent["ws19"]
        print("decode-only path, unfused launches: kind 19 equals variant 2, its workspace grows; kind 12 unchanged")
    else:
        torch.save({"kind12": out.cpu(), "variant2": tail(m, mid(m, y8, 2)).cpu(), "ws19": ws19}, tmp_path / "parent.pt")


def test_decode_only_path_with_the_unfused_knob(tmp_path):
    """The library reads its debug knobs once per process, so the test above is re-run in a child process with the knob set."""
    test_decode_only_path_and_kind_12(tmp_path)
    env = dict(os.environ, AUXRESCONV_PARENT_OUTPUTS=str(tmp_path / "parent.pt"), **KNOB_ENV)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "decode_only_path_and_kind_12"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "kind 12 unchanged" in r.stdout, r.stdout[-500:]


# ---- 4. the engine's trajectory, replay == eager, resume ----------------------------------------------------------------------------
def test_engine_trajectory_against_the_reference(golden_dir):
    G.engine_trajectory_against_the_reference(FAMILY, golden_dir, "vae_traj_auxresconv", "auxresconv", steps=4)


def test_replay_equals_eager_and_resume_continues_to_the_same_bits():
    """One optimiser with a weight average: the captured step replays through the beta ramp, the checkpoint carries the average"""
    nd, z, c, B = 5, 8, 40, 8
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(nd, z, c, True).state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer="adam", lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg="polyak", weight_avg_start=1)
    a, _, _ = G.replay_equals_eager_and_resume(lambda: build(nd, z, c, True, sd0), xs, cfg, resume_at=3)
    assert torch.equal(a.eps, G.aux_draws(B, nd, z, 99, a.RNG_STRIDE * a.step_count))


# ---- 5. IWAE evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    G.iwae_on_injected_draws(FAMILY, golden_dir, "vae_" + case, case)


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    """200 images at k = 4: one chunk against chunks of 64.  Every call runs on fixed groups (64 images for the statistics and the ELBO pass, 16 for the
    stages and the decoder), so elbo and logprob are equal to the bit."""
    N, k, nd, zd = 200, 4, 10, 6
    m = seeded(nd, zd, 42, True, 8)
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    G.iwae_does_not_depend_on_the_chunking(FAMILY, m, x, k, [(None, [200]), (100, [64, 64, 64, 8])])
