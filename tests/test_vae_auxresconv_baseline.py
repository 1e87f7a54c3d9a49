"""The hierarchical resconv Gaussian baseline (ardae_model_desc.kind 19, the reference's `vae.py --model auxresconv` / `auxresconvct`): layout, descriptor
rules and argument validation through the C ABI (ardae_resconv_mid included), the module surface, the evaluator's plan, the decode-only workspace, and
the float64 torch restatement of the family - ONE weight-normalised trunk, the two concatenations with ctx FIRST, both KLs, the three-stage logprob, and
the decoder's 14 x 14 stage on its own - that the GPU tests lean on, pinned here to the reference's float64 fixtures.  No GPU needed.

The fixtures (tools/gen_vae_golden.py, family auxresconv) do not store the parameters: `auxres_params` regenerates them from the stored seed with the
recipe the tool called (oracle.fixture_params.auxresconv)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import ardae_oracle as O
from oracle import fixture_params as P
import vae_restate as R
from vae_restate import BETAS, TOL64, fails, kld_rows, lin, load, log_normal_rows, pair_kld_rows, rel, relaxed_sample
from vae_restate import resconv_decode_logit as decode_logit
from vae_restate import resconv_tail_logit as tail_logit

CASES = ("auxresconv_n100_z32_c450_b3", "auxresconv_n10_z6_c42_b5")
D = 784
ELU = 3               # ARDAE_ACT_ELU


def shape_of(fx):
    """-> (B, noise, z, c_dim), do_center"""
    return tuple(int(v) for v in fx["shape"]), bool(int(fx["do_center"]))


def auxres_params(fx, dtype=torch.float32):
    """The recipe tools/gen_vae_golden.py called: oracle.fixture_params.auxresconv (the float64 runs start from the fp32 numbers, widened)"""
    (_, nd, z, c), _ = shape_of(fx)
    return {k: v.to(dtype) for k, v in P.auxresconv(nd, z, c, int(fx["seed"])).items()}


def desc_of(nd, z, c, center):
    return L.ModelDesc(19, D, nd, c, z, 1, ELU, 0 if center else L.MODEL_NO_CENTER)


# ---- the test-side oracle: the family restated in plain torch (trunk and decoder: vae_restate) ---------------------------------------
def trunk(p, center, x):
    """InputEncoder.forward (vae/auxresconv.py:52-63) -> ctx [B, c_dim]"""
    return R.resconv_trunk(p, "inp_encode.enc.", center, x)


def head(p, prefix, h):
    return lin(p, prefix + "reparam.mean_fn", h), lin(p, prefix + "reparam.logvar_fn", h)


def cat_stats(p, prefix, ctx, s, k=1):
    """-> (mean, logvar) of encode / aux_decode: fc.0 + ELU on cat[ctx, s] with ctx FIRST and each image's ctx repeated for its k rows of s"""
    return head(p, prefix, F.elu(lin(p, prefix + "fc.0", torch.cat([ctx.repeat_interleave(k, 0), s], 1))))


def forward(p, center, x, eps, beta):
    """-> dict(mu0, lv0, z, mean, logit, loss, recon, kld): VAE.forward (vae/auxresconv.py:310-340); kld = kld + aux_kld"""
    nd = p["aux_encode.reparam.mean_fn.weight"].size(0)
    ctx = trunk(p, center, x)
    mu0, lv0 = head(p, "aux_encode.", ctx)
    z0 = mu0 + torch.exp(0.5 * lv0) * eps[:, :nd]
    mu, lv = cat_stats(p, "encode.", ctx, z0)
    z = mu + torch.exp(0.5 * lv) * eps[:, nd:]
    mup, lvp = cat_stats(p, "aux_decode.", ctx, z)
    rec, logit = R.resconv_recon_rows(p, x, z)
    kld, aux = kld_rows(mu, lv), pair_kld_rows(mu0, lv0, mup, lvp)
    return dict(mu0=mu0, lv0=lv0, z=z, mean=torch.sigmoid(logit), logit=logit, loss=(rec + beta * kld + beta * aux).mean(), recon=rec.mean(),
                kld=(kld + aux).mean())


loss_and_grads = functools.partial(R.loss_and_grads, forward)      # (p, center, x, eps, beta, scale=) -> forward's dict (detached), {name: gradient}


def logq_rows(p, center, x, eps):
    """The three stochastic stages of VAE.logprob (vae/auxresconv.py:357-394, sample_size2 = 1) on injected draws eps [B, k, noise + z]
    -> z [B k, zd], logq [B k] = log q(z0|x) + log q(z|z0,x) - log r(z0|z,x)"""
    B, k, _ = eps.shape
    nd = p["aux_encode.reparam.mean_fn.weight"].size(0)
    ctx = trunk(p, center, x)
    mu0, lv0 = (v.repeat_interleave(k, 0) for v in head(p, "aux_encode.", ctx))
    e = eps.reshape(B * k, -1)
    z0 = mu0 + torch.exp(0.5 * lv0) * e[:, :nd]
    mu, lv = cat_stats(p, "encode.", ctx, z0, k)
    z = mu + torch.exp(0.5 * lv) * e[:, nd:]
    mup, lvp = cat_stats(p, "aux_decode.", ctx, z, k)
    return z, log_normal_rows(z0, mu0, lv0) + log_normal_rows(z, mu, lv) - log_normal_rows(z0, mup, lvp)


def logprob_rows(p, center, x, eps):
    """VAE.logprob before its mean, [B]"""
    B, k, _ = eps.shape
    z, logq = logq_rows(p, center, x, eps)
    rec, _ = R.resconv_recon_rows(p, x.repeat_interleave(k, 0), z)
    return R.iw_logsumexp((-rec + log_normal_rows(z, torch.zeros_like(z), torch.zeros_like(z)) - logq).view(B, k))


def head_map(p, z):
    """decode.dec.0 .. decode.dec.8 on z [R, zd] -> y8 [R, 8, 8, 32] NHWC, dec.8's output after its ELU (what ardae_resconv_mid reads)"""
    h = F.elu(O.res_linear(p, "decode.dec.0.", z, True))
    h = F.elu(O.res_linear(p, "decode.dec.2.", h, True)).view(-1, 32, 4, 4)
    h = F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=True)
    h = F.elu(O.res_conv(p, "decode.dec.6.", h, 1, F.elu))
    return F.elu(O.res_conv(p, "decode.dec.8.", h, 1, F.elu)).permute(0, 2, 3, 1)


def mid_map(p, y8):
    """The decoder's 14 x 14 stage on y8 [R, 8, 8, 32] NHWC: the crop [:, :, :-1, :-1], the x2 upsampling, decode.dec.12 + ELU, decode.dec.14 + ELU
    -> y14 [R, 14, 14, 16] NHWC (what ardae_resconv_tail reads)"""
    u = F.interpolate(y8.permute(0, 3, 1, 2)[:, :, :-1, :-1], scale_factor=2, mode="bilinear", align_corners=True)
    h = F.elu(O.res_conv(p, "decode.dec.12.", u, 1, F.elu))
    return F.elu(O.res_conv(p, "decode.dec.14.", h, 1, F.elu)).permute(0, 2, 3, 1)


def restate(fx):
    """-> the fixture's parameters in float64, cfg (do_center)"""
    return auxres_params(fx, torch.float64), shape_of(fx)[1]


def trajectory(fx):
    """The fixture's loop restated in float64: yields (step, forward's dict, the parameters after the vendored Adam's step)"""
    p, center = restate(fx)
    return R.trajectory(fx, p, lambda p, x, eps, beta: loss_and_grads(p, center, R.t64(x), R.t64(eps), beta, scale=1.0 / D))


# ---- 1. the restatement, pinned to the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference_in_float64(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    p, center = restate(fx)
    x, eps, dec = (R.t64(fx[k]) for k in ("x", "eps", "dec_noise"))
    for b, beta in BETAS.items():
        out, grads = loss_and_grads(p, center, x, eps, beta, scale=1.0 / D)
        for k in ("z", "mean", "loss", "recon", "kld"):
            assert rel(out[k], fx[f"{b}/{k}_f64"]) <= TOL64, (b, k)
        assert rel(relaxed_sample(out["logit"], dec), fx[f"{b}/x_sample_f64"]) <= TOL64
        assert rel(out["mu0"], fx["mu0_f64"]) <= TOL64 and rel(out["lv0"], fx["lv0_f64"]) <= TOL64
        R.check_grads_f64(grads, fx, b, TOL64, params=p)
    lp = logprob_rows(p, center, x, R.t64(fx["lp/eps"])).mean()
    assert rel(lp, fx["lp/value_f64"]) <= TOL64
    # the fp32 fixture is the same computation at fp32's precision
    assert rel(fx["b1/loss"], fx["b1/loss_f64"]) <= 1e-5 and rel(fx["lp/value"], fx["lp/value_f64"]) <= 1e-5


def test_restated_trajectory_is_the_reference_in_float64(golden_dir):
    fx = load(golden_dir, "vae_traj_auxresconv")
    assert int(fx["cfg/steps"]) == 4
    R.check_traj_f64(trajectory(fx), fx, TOL64)
    assert float(fx["1/beta"]) < 1.0 == float(fx["2/beta"]) == float(fx["3/beta"])          # the ramp ends inside the run


def test_mid_stage_restatement_is_the_decoder_in_float64(golden_dir):
    """head_map -> mid_map -> the last stage is the oracle's decoder: the pieces the GPU test compares ardae_resconv_mid against"""
    fx = load(golden_dir, "vae_" + CASES[1])
    p = auxres_params(fx, torch.float64)
    z = torch.randn(3, 6, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    y8 = head_map(p, z)
    y14 = mid_map(p, y8)
    assert y8.shape == (3, 8, 8, 32) and y14.shape == (3, 14, 14, 16)
    assert rel(tail_logit(p, y14), decode_logit(p, z)) <= 1e-14
    # the cropped strip (row 7 and column 7 of y8) is never read
    y8n = y8.clone()
    y8n[:, 7, :, :] = float("nan"); y8n[:, :, 7, :] = float("nan")
    assert torch.equal(mid_map(p, y8n), y14)
    # the border outputs (index 0 and 13) interpolate from source index 0 and 6 alone
    u = F.interpolate(y8.permute(0, 3, 1, 2)[:, :, :-1, :-1], scale_factor=2, mode="bilinear", align_corners=True)
    assert torch.equal(u[:, :, 13, 13], y8[:, 6, 6, :]) and torch.equal(u[:, :, 0, 13], y8[:, 0, 6, :])


# ---- 2. layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + ("traj_auxresconv",))
def test_spec_names_and_shapes_are_the_fixtures(golden_dir, name):
    fx = load(golden_dir, "vae_" + name)
    (B, nd, z, c), center = shape_of(fx)
    assert str(fx["act"]) == "elu"
    spec = layout.aux_resconv_vae_spec(nd, z, c)
    assert [n for n, _ in spec] == [str(n) for n in fx["names"]]
    assert [",".join(str(d) for d in s) for _, s in spec] == [str(s) for s in fx["shapes"]]
    assert spec[0][0] == "inp_encode.enc.0.conv_0h.direction" and spec[-1][0] == "aux_decode.reparam.logvar_fn.bias"
    order = [n.split(".")[0] + "." + n.split(".")[1] for n, _ in spec]
    assert list(dict.fromkeys(order)) == ["inp_encode.enc", "aux_encode.reparam", "encode.fc", "encode.reparam", "decode.dec", "aux_decode.fc",
                                          "aux_decode.reparam"]
    desc = desc_of(nd, z, c, center)
    total = layout.offsets(spec)[1]
    assert total == L.query("ardae_model_param_floats", desc) == sum(v.numel() for v in auxres_params(fx).values())
    assert L.query("ardae_model_packed_floats", desc) > total
    mod = net.MNISTResConvAuxVAE(z0_dim=nd, z_dim=z, c_dim=c, do_center=center)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [(n, tuple(s)) for n, s in spec]
    sd = auxres_params(fx)
    mod.load_state_dict(sd)
    assert torch.equal(mod.flat_params(), torch.cat([v.reshape(-1) for v in sd.values()]))
    assert (mod._desc.kind, mod._desc.flags, mod._desc.noise_dim, mod._desc.h_dim, mod._desc.n_layers) == (19, 0 if center else L.MODEL_NO_CENTER, nd, c, 1)


def test_parameter_count_at_the_recipe_widths(golden_dir):
    counts = load(golden_dir, "vae_auxresconv_param_counts")
    assert sorted(counts) == ["auxresconv_100_32_450"]
    d = desc_of(100, 32, 450, False)
    spec = layout.aux_resconv_vae_spec(100, 32, 450)
    assert layout.offsets(spec)[1] == L.query("ardae_model_param_floats", d) == int(counts["auxresconv_100_32_450"]) == 2459187
    assert len(spec) == 133
    assert sum(p.numel() for p in net.MNISTResConvAuxVAE().parameters()) == 2459187
    assert net.modules.KIND_IDS["vae_auxresconv"] == 19
    # the z head has kind 12's policy: the unfused launches are the default at every width
    assert [L.query("ardae_vae_head_fused_ok", desc_of(100, z, c, False)) for z, c in ((32, 450), (6, 42), (32, 448), (65, 450))] == [0, 0, 0, 0]


# ---- 3. descriptor rules and refusals, before any HIP call --------------------------------------------------------------------------
one, big, small = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40), ctypes.c_size_t(16)      # any non-null address: validation fails before it is read
ref = ctypes.byref


def desc(**kw):
    return L.ModelDesc(*[kw.get(k, v) for k, v in (("kind", 19), ("input_dim", 784), ("noise_dim", 1), ("h_dim", 1), ("z_dim", 1), ("n_layers", 1),
                                                    ("act", ELU), ("flags", 0))])


def test_descriptor_rules():
    lib = L.lib()
    ok = desc()                                                            # the smallest descriptor
    assert lib.ardae_model_param_floats(ref(ok)) > 0 and lib.ardae_model_packed_floats(ref(ok)) > lib.ardae_model_param_floats(ref(ok))
    assert all(lib.ardae_model_workspace_floats(ref(ok), 3, 1, mode) > 0 for mode in (0, 1, 2))
    fails(lib.ardae_model_pack(ref(ok), one, None, None), "null pointer")
    assert lib.ardae_model_param_floats(ref(desc(noise_dim=128, z_dim=200, h_dim=450, flags=L.MODEL_NO_CENTER))) > 0
    for bad, why in ((desc(input_dim=783), "input_dim 784"), (desc(h_dim=0), "bad dimensions"), (desc(n_layers=2), "n_layers must be 1"),
                     (desc(noise_dim=0), "noise_dim must be 1 .. 128"), (desc(noise_dim=129), "noise_dim must be 1 .. 128"),
                     (desc(noise_dim=-1), "noise_dim must be 1 .. 128"), (desc(flags=2), "flags must be 0 or ARDAE_MODEL_NO_CENTER"),
                     (desc(flags=4 << L.MODEL_CLIP_Z0_SHIFT), "flags must be 0 or ARDAE_MODEL_NO_CENTER"), (desc(z_dim=0), "bad dimensions"),
                     (desc(act=0), "ELU only"), (desc(act=1), "ELU only"), (desc(act=99), "ELU only")):
        assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_packed_floats(ref(bad)) == 0
        assert all(lib.ardae_model_workspace_floats(ref(bad), 4, 1, mode) == 0 for mode in (0, 1, 2))
        assert lib.ardae_model_workspace_floats(ref(bad), 4, 16, 4) == 0
        assert lib.ardae_resconv_mid_workspace_floats(ref(bad), 4, 2) == 0 and lib.ardae_vae_head_fused_ok(ref(bad)) == 0
        assert lib.ardae_resconv_tail_workspace_floats(ref(bad), 4, 2) == 0
        fails(lib.ardae_model_pack(ref(bad), one, one, None), why)
    # 18 is no kind, as 10, 13 and 16 are not; 20 neither
    for k in (18, 20):
        bad = desc(kind=k)
        assert lib.ardae_model_param_floats(ref(bad)) == 0
        fails(lib.ardae_model_pack(ref(bad), one, one, None), "kind must be")
        assert b"17 (MNISTConvAuxVAE), or 19 (MNISTResConvAuxVAE)" in lib.ardae_last_error()
        fails(lib.ardae_vae_encode_stats(ref(bad), one, one, one, 4, one, big, one, one, None), "kind must be")
        assert b"17 (MNISTConvAuxVAE), or 19 (MNISTResConvAuxVAE)" in lib.ardae_last_error()
    # the workspace modes: one draw per image, no sampler pair; the evaluation pass grows with B and k
    d = desc(noise_dim=10, z_dim=6, h_dim=42)
    ws = lambda B, nz, mode: lib.ardae_model_workspace_floats(ref(d), B, nz, mode)      # noqa: E731
    assert ws(4, 2, 0) == ws(4, 2, 1) == ws(4, 1, 3) == 0
    assert ws(4, 1, 1) > ws(4, 1, 0) > 0
    assert 0 < ws(4, 8, 4) < ws(4, 16, 4) < ws(9, 16, 4) < ws(70, 16, 4)
    for per_mode in ([ws(b, 1, mode) for b in (1, 9, 70)] for mode in (0, 1, 2)):
        assert 0 < per_mode[0] < per_mode[1] < per_mode[2]
    assert ws(64, 4, 2) == ws(256, 1, 2)


def test_decode_only_workspace_is_below_kind_12s_at_equal_widths():
    """Mode 2 of kind 19 drops c7, u14 and the buffers of dec[4] / dec[5] but dec[5]'s output, and sizes the one columns scratch from the 8 x 8 blocks
    (2 x 64 x 288 floats a row in place of 196 x 288 + 196 x 144).  From the carving at c_dim 450: 36 864 columns + 2 x 450 + 2 x 512 + 512 + 2048
    + 4 x 2048 + 3136, each rounded up to 64 floats per call, ~5.3e4 a row against kind 12's 117 732."""
    for z, c in ((32, 450), (6, 42)):
        d19, d12 = desc_of(100, z, c, False), L.ModelDesc(12, D, 0, c, z, 1, ELU, L.MODEL_NO_CENTER)
        for R in (1, 256, 4096):
            w19, w12 = L.query("ardae_model_workspace_floats", d19, R, 1, 2), L.query("ardae_model_workspace_floats", d12, R, 1, 2)
            print(f"mode-2 floats per decoded row at R = {R}, c_dim {c}: kind 19 {w19 / R:.0f}, kind 12 {w12 / R:.0f}")
            assert 0 < w19 < w12 and 2 * w19 < w12
    per_row = L.query("ardae_model_workspace_floats", desc_of(100, 32, 450, False), 4096, 1, 2) / 4096
    assert 52000 < per_row < 54000
    assert L.query("ardae_model_workspace_floats", L.ModelDesc(12, D, 0, 450, 32, 1, ELU, L.MODEL_NO_CENTER), 4096, 1, 2) / 4096 > 117000
    # the unfused launches' own buffers, and none for the kernel
    d = desc_of(100, 32, 450, False)
    assert L.query("ardae_resconv_mid_workspace_floats", d, 3, 1) == L.query("ardae_resconv_mid_workspace_floats", d, 3, 0) == 0
    assert L.query("ardae_resconv_mid_workspace_floats", d, 3, 2) >= 3 * (49 * 32 + 196 * 32 + 196 * (288 + 144 + 32) + 196 * (144 + 144 + 32))


def test_argument_validation_of_every_entry_point():
    lib = L.lib()
    fwd = lambda d, x, B, wsf, z, losses: lib.ardae_vae_forward(ref(d), one, one, x, None, B, 1.0, 1.0, 7, 0, None, one, wsf, z, None, losses, None)
    fwd_dev = lambda d, st: lib.ardae_vae_forward_dev(ref(d), one, one, one, None, 4, st, 1.0, 7, 0, None, one, big, one, None, one, None)
    bwd = lambda d, B, wsf, g: lib.ardae_vae_backward(ref(d), one, one, one, B, 1.0, 1.0, one, wsf, g, 0.0, None)
    bwd_dev = lambda d, st: lib.ardae_vae_backward_dev(ref(d), one, one, one, 4, st, 1.0, one, big, one, 0.0, None)
    stats_ = lambda d, B, wsf, mu, lv: lib.ardae_vae_encode_stats(ref(d), one, one, one, B, one, wsf, mu, lv, None)
    head_ = lambda d, B, variant, mu, eps_out=one: lib.ardae_vae_head(ref(d), one, one, one, None, B, 7, 0, None, variant, mu, one, one, eps_out, one, None)
    draw = lambda d, x, B, k, first, wsf, z, lq, eps=None: lib.ardae_vae_aux_iwae_draw(ref(d), one, one, x, one, one, eps, B, k, 7, 0, 1, first, one, wsf, z, lq,
                                                                                       None, None)
    elbo = lambda d, x, B, first, wsf, rec, kld, eps=None: lib.ardae_vae_aux_elbo_rows(ref(d), one, one, x, eps, B, 7, 0, 1, first, one, wsf, rec, kld, None)
    ok = desc(noise_dim=3, z_dim=5, h_dim=7)
    bad, why = desc(noise_dim=0, z_dim=5, h_dim=7), "noise_dim must be"
    for rc in (fwd(bad, one, 4, big, one, one), bwd(bad, 4, big, one), stats_(bad, 4, big, one, one), head_(bad, 4, 0, one)):
        fails(rc, why)
    fails(draw(bad, one, 4, 16, 0, big, one, one), why)
    fails(elbo(bad, one, 4, 0, big, one, one), why)
    fails(lib.ardae_model_decode(ref(bad), one, one, one, 4, one, big, one, None, None), why)
    fails(fwd(ok, one, 0, big, one, one), "bad batch")
    fails(fwd(ok, one, -3, big, one, one), "bad batch")
    fails(fwd(ok, one, 4, small, one, one), "workspace too small")
    fails(fwd(ok, None, 4, big, one, one), "null pointer")
    fails(fwd(ok, one, 4, big, None, one), "null pointer")
    fails(fwd(ok, one, 4, big, one, None), "null pointer")
    fails(fwd_dev(ok, None), "beta_state is NULL")
    fails(bwd(ok, 0, big, one), "bad batch")
    fails(bwd(ok, 4, small, one), "workspace too small")
    fails(bwd(ok, 4, big, None), "null pointer")
    fails(bwd_dev(ok, None), "beta_state is NULL")
    fails(stats_(ok, 0, big, one, one), "bad batch")
    fails(stats_(ok, 4, small, one, one), "workspace too small")
    fails(stats_(ok, 4, big, None, one), "null pointer")
    fails(stats_(ok, 4, big, one, None), "null pointer")
    fails(head_(ok, 0, 1, one), "bad batch")
    fails(head_(ok, 4, 3, one), "variant must be")
    fails(head_(ok, 4, 1, None), "null pointer")
    fails(head_(ok, 4, 2, one, eps_out=None), "null pointer")
    fails(head_(desc(noise_dim=3, z_dim=65, h_dim=7), 4, 1, one), "the fused head takes")
    fails(lib.ardae_model_decode(ref(ok), one, one, one, 4, one, small, one, None, None), "workspace too small")
    fails(lib.ardae_model_decode(ref(ok), one, one, None, 4, one, big, one, None, None), "bad arguments")
    # the two aux entry points
    fails(draw(ok, one, 0, 16, 0, big, one, one), "bad batch")
    fails(draw(ok, one, 4, 0, 0, big, one, one), "bad batch")
    fails(draw(ok, one, 1 << 20, 1 << 12, 0, big, one, one), "bad batch")
    fails(draw(ok, one, 4, 16, 0, small, one, one), "workspace too small")
    fails(draw(ok, None, 4, 16, 0, big, one, one), "null pointer")
    fails(draw(ok, one, 4, 16, 0, big, None, one), "null pointer")
    fails(draw(ok, one, 4, 16, 0, big, one, None), "null pointer")
    fails(draw(ok, one, 4, 3, 1, big, one, one), "multiples of 4")                        # 1 x 3 x 3 normals before the chunk: no whole counter
    fails(draw(ok, one, 4, 3, 1, small, one, one, eps=one), "workspace too small")        # ... which injected draws do not need
    fails(draw(desc(noise_dim=3, z_dim=129, h_dim=7), one, 4, 16, 0, big, one, one), "z_dim <= 128")
    fails(elbo(ok, one, 0, 0, big, one, one), "bad batch")
    fails(elbo(ok, one, 4, 0, small, one, one), "workspace too small")
    fails(elbo(ok, None, 4, 0, big, one, one), "null pointer")
    fails(elbo(ok, one, 4, 0, big, None, one), "null pointer")
    fails(elbo(ok, one, 4, 0, big, one, None), "null pointer")
    fails(elbo(ok, one, 4, 2, big, one, one), "multiples of 4")
    # their kind message keeps the earlier fragment and names the new kind
    for other in (L.ModelDesc(12, 784, 0, 450, 4, 1, ELU, 0), L.ModelDesc(6, 784, 3, 450, 4, 1, ELU, 0), desc(kind=18)):
        for rc in (draw(other, one, 4, 16, 0, big, one, one), elbo(other, one, 4, 0, big, one, one)):
            fails(rc, "kind must be 14 (MNISTAuxVAE) or 15 (ToyAuxVAE) or 17 (MNISTConvAuxVAE) or 19 (MNISTResConvAuxVAE)")
    # the implicit models' calls refuse the family: there is no sampler
    fails(lib.ardae_model_encode(ref(ok), one, one, one, None, 4, 1, one, big, one, None), "analytic posterior")
    fails(lib.ardae_model_vae_forward(ref(ok), one, one, one, one, 4, 1, 1.0, one, big, one, one, None), "ardae_vae_forward")
    fails(lib.ardae_model_vae_backward(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, None, one, big, one, 0.0, None), "ardae_vae_backward")
    fails(lib.ardae_model_vae_backward_decoder(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, one, big, None), "no split backward")
    fails(lib.ardae_model_encode_hidden(ref(ok), one, one, one, 4, one, big, one, None, None), "hidden1a context")


def test_argument_validation_of_resconv_mid_and_tail():
    lib = L.lib()
    mid = lambda d, R, variant, y8=one, ws=one, wsf=big, out=one, params=one, packed=one: lib.ardae_resconv_mid(ref(d), params, packed, y8, R, variant, ws,
                                                                                                                wsf, out, None)
    ok = desc(noise_dim=3, z_dim=5, h_dim=7)
    fails(lib.ardae_resconv_mid(None, one, one, one, 4, 1, one, big, one, None), "desc is NULL")
    for variant in (-1, 3):
        fails(mid(ok, 4, variant), "variant must be")
        assert lib.ardae_resconv_mid_workspace_floats(ref(ok), 4, variant) == 0
    for R in (0, -2, 1 << 20):
        fails(mid(ok, R, 1), "bad batch")
        assert lib.ardae_resconv_mid_workspace_floats(ref(ok), R, 2) == 0
    fails(mid(ok, 4, 1, y8=None), "null pointer")
    fails(mid(ok, 4, 1, out=None), "null pointer")
    fails(mid(ok, 4, 1, params=None), "null pointer")
    fails(mid(ok, 4, 1, packed=None), "null pointer")
    fails(mid(ok, 4, 2, ws=None), "need a workspace")                     # variant 2 without a workspace
    fails(mid(ok, 4, 2, wsf=small), "workspace too small")
    fails(mid(desc(noise_dim=3, z_dim=5, h_dim=7, act=1), 4, 1), "ELU only")
    assert lib.ardae_resconv_mid_workspace_floats(None, 4, 2) == 0
    for other in (L.ModelDesc(12, 784, 0, 450, 5, 1, ELU, 0), L.ModelDesc(6, 784, 3, 450, 5, 1, ELU, 0), L.ModelDesc(17, 784, 3, 800, 5, 1, 2, 0)):
        fails(mid(other, 4, 1), "kind must be 19 (MNISTResConvAuxVAE)")
        assert lib.ardae_resconv_mid_workspace_floats(ref(other), 4, 2) == 0
    # ardae_resconv_tail takes the kind as it takes kind 12; its message keeps the earlier fragment
    tail = lambda d, R, variant, ws=one, wsf=big: lib.ardae_resconv_tail(ref(d), one, one, one, R, variant, ws, wsf, one, None)      # noqa: E731
    assert lib.ardae_resconv_tail_workspace_floats(ref(ok), 4, 1) == 0 < lib.ardae_resconv_tail_workspace_floats(ref(ok), 4, 2)
    fails(tail(ok, 4, 3), "variant must be")
    fails(tail(ok, 4, 2, ws=None), "need a workspace")
    fails(tail(ok, 4, 2, wsf=small), "workspace too small")
    fails(tail(desc(noise_dim=0, z_dim=5, h_dim=7), 4, 1), "noise_dim must be")
    for other in (L.ModelDesc(6, 784, 3, 450, 5, 1, ELU, 0), L.ModelDesc(11, 784, 0, 800, 5, 1, 2, 0)):
        fails(tail(other, 4, 1), "kind must be 12 (MNISTResConvVAE)")


# ---- 4. the module surface -----------------------------------------------------------------------------------------------------------
def test_module_surface_and_refusals():
    torch.manual_seed(0)
    m = net.MNISTResConvAuxVAE()
    assert (m.input_height, m.input_channels, m.z0_dim, m.noise_dim, m.h_dim, m.c_dim, m.z_dim, m.nonlinearity, m.do_center, m.input_dim) == \
        (28, 1, 100, 100, 450, 450, 32, "elu", False, 784)
    assert isinstance(m, net.GaussianVAE) and m.latent_dim == 32 and m._eps_width == 132 and m.return_samples and m._eval_groups[0] % 4 == 0
    assert m._desc.flags == L.MODEL_NO_CENTER and net.MNISTResConvAuxVAE(z0_dim=5, z_dim=4, c_dim=9, do_center=True)._desc.flags == 0
    p = {k: v.detach() for k, v in m.named_parameters()}
    # the weight-normalised operators as kinds 6 / 12: scale 1, direction and bias U(+-1/sqrt(in)); the plain Linears torch's default
    assert float(p["inp_encode.enc.4.conv_h1.scale"].min()) == float(p["decode.dec.12.conv_01.scale"].max()) == 1.0
    for k, fan_in in (("inp_encode.enc.2.conv_0h", 16), ("inp_encode.enc.11.dot_01", 512), ("decode.dec.0.dot_0h", 32), ("decode.dec.12.conv_0h", 32)):
        bound = 1.0 / math.sqrt(fan_in)
        assert 0.9 * bound < float(p[k + ".direction"].abs().max()) <= bound and 0.0 < float(p[k + ".bias"].abs().max()) <= bound, k
    for k, fan_in in (("encode.fc.0", 550), ("aux_decode.fc.0", 482), ("aux_encode.reparam.mean_fn", 450), ("encode.reparam.logvar_fn", 450),
                      ("aux_decode.reparam.logvar_fn", 450)):
        bound = 1.0 / math.sqrt(fan_in)
        assert 0.9 * bound < float(p[k + ".weight"].abs().max()) <= bound and 0.0 < float(p[k + ".bias"].abs().max()) <= bound, k
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTResConvAuxVAE(input_height=32)
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTResConvAuxVAE(input_channels=2)
    with pytest.raises(NotImplementedError, match="asserts 'elu'"):
        net.MNISTResConvAuxVAE(nonlinearity="softplus")
    with pytest.raises(NotImplementedError, match="normal_energy_func"):
        net.MNISTResConvAuxVAE(energy_func=lambda z: z.sum(1))
    for bad in (0, 129):
        with pytest.raises(ValueError, match="noise_dim must be 1 .. 128"):
            net.MNISTResConvAuxVAE(z0_dim=bad)
    m5 = net.MNISTResConvAuxVAE(z0_dim=5, z_dim=4, c_dim=9)
    for call in (lambda: m5(torch.zeros(3, 784)), lambda: m5(torch.zeros(3, 1, 28, 28)), lambda: m5.logprob(torch.zeros(3, 784), sample_size=4),
                 lambda: m5.logprob_rows(torch.zeros(3, 784), 4), lambda: m5.encode_stats(torch.zeros(3, 784)), lambda: m5.generate(2),
                 lambda: m5.decode_params(torch.zeros(3, 4))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.VaeEngine(m5, net.VaeConfig(), batch_size=4)
    # the engine / evaluator type checks keep naming the existing classes in order, and name the new one last
    with pytest.raises(TypeError, match="VaeEngine drives.*net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE.*net.MNISTAuxVAE / "
                                        r"net.ToyAuxVAE / net.MNISTConvAuxVAE / net.MNISTResConvAuxVAE\)"):
        net.VaeEngine(net.MNISTResConvAuxIPVAE(), net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE.*net.ToyAuxVAE / net.MNISTConvAuxVAE / "
                                        "net.MNISTResConvAuxVAE "):
        net.GaussianIwaeEvaluator(net.MNISTResConvAuxIPVAE(), 16)
    with pytest.raises(NotImplementedError, match="z_dim 129 > 128"):
        net.GaussianIwaeEvaluator(net.MNISTResConvAuxVAE(z0_dim=5, z_dim=129, c_dim=9), 16)


def test_evaluator_plans_whole_groups_within_the_default_budget():
    ev = net.GaussianIwaeEvaluator(net.MNISTResConvAuxVAE(), 256)
    assert ev.aux and ev.sd == 100 and not ev.gaussian
    G, g = ev.image_group, ev.group
    assert (G, g) == net.MNISTResConvAuxVAE._eval_groups == (64, 16) and G % g == 0 and g % 4 == 0
    plan = ev.plan(2048)
    assert plan[0][0] == 0 and plan[-1][1] == 2048 and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
    assert all((b - a) % G == 0 for a, b in plan[:-1]) and ev.floats_per_chunk(plan[0][1]) <= ev.budget == 1 << 28
    # the group of the importance samples' decoder is sized from the fused carve: g is the largest group whose g * 256 rows fit the budget
    d = ev.model._desc
    assert L.query("ardae_model_workspace_floats", d, g * 256, 1, 2) < ev.budget < L.query("ardae_model_workspace_floats", d, 2 * g * 256, 1, 2)
    small_ = net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(150))
    assert [b - a for a, b in small_.plan(300)] == [64, 64, 64, 64, 44]       # cut down to whole groups
    with pytest.raises(ValueError, match="one group of 64 images"):
        net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(40)).plan(100)
    assert net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(12)).plan(12) == [(0, 12)]
