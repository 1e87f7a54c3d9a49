"""The image-model families of the shipped dbMNIST recipes (run_vae_dbmnist.sh: --train-batch-size 128 --train-nz-cdae 625) at the
recipes' own batch, against the oracle run live on the CPU.

The batch decides which kernels run.  At the 4 images of the *_b4_nz8 fixtures every conv / transposed-conv product fits
`linear_small` and most weight gradients `wgrad_small_kernel`; at 128 images the 14x14 and 28x28 blocks (25,088 / 100,352 rows) and
ConvIPVAE's decoder go to the generic `linear_kernel<...>` (ELU epilogues, two-source skips, DACT backward epilogues), every conv weight
gradient to `wgrad_kernel` with its row splits and split reduction, and the gather / scatter kernels (im2col / col2im, upsampling,
crop-pad, layout changes, spm4) run on grids 32x larger.  This module checks that path:

  1. the VAE phase at 128 images against the oracle in float64: losses, encoder / context / decoder outputs and EVERY gradient tensor,
     each bounded by a backstop and by a multiple of the fp32 oracle's own error;
  2. the kernels that ran (so that a change of the dispatch thresholds cannot quietly turn this back into a `linear_small` test);
  3. the IWAE bound at the recipes' --iws-samples (256 / 1024: the decoder on k images);
  4. whole teacher-forced steps at the exact recipe shape (128 x 625, the recipe's cDAE, optimisers and --num-cdae-updates).
"""
import ctypes
import os
import statistics

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O
from test_engine_gpu import RES_RECIPE, _oracle_opt_state, assert_update_close, build, rel, rel_l2, train_config

pytestmark = pytest.mark.gpu

B = 128            # --train-batch-size
NZ = 625           # --train-nz-cdae
RES_CDAE = O.CdaeCfg("res", 32, 32, 512, 5)        # --cdae mlp-res --cdae-h-dim 512 --cdae-n-layers 5 (context width set per family)
GRAD_CDAE = O.CdaeCfg("grad", 32, 32, 256, 5)      # --cdae mlp-grad --cdae-h-dim 256 --cdae-n-layers 5

# model, cDAE context width, cDAE.  The recipes: resconvct-res (res-wn-mlp head, h 512, 1 layer; its 'mlp'-head twin resconvct),
# auxresconvct (c_dim 450) and auxresconvct-clip, mnist-conv, auxconv, auxmnist (hidden widths 300, 2 layers)
FAMILIES = {
    "resconv": (O.ModelCfg("resconv", 784, 100, 512, 32, 1, "elu"), 32, RES_CDAE),
    "resconv_mlp": (O.ModelCfg("resconv", 784, 100, 512, 32, 1, "elu", enc_type="mlp"), 32, RES_CDAE),
    "auxresconv": (O.ModelCfg("auxresconv", 784, 100, 450, 32, 1, "elu"), 450, RES_CDAE),
    "auxresconv_clip": (O.ModelCfg("auxresconv", 784, 100, 450, 32, 1, "elu", clipped=True), 450, RES_CDAE),
    "conv": (O.ModelCfg("conv", 784, 100, 800, 32, 1, "softplus"), 32, GRAD_CDAE),
    "auxconv": (O.ModelCfg("auxconv", 784, 100, 800, 32, 1, "softplus"), 1600, GRAD_CDAE),
    "auxmnist": (O.ModelCfg("auxmnist", 784, 100, 300, 32, 2, "softplus"), 600, GRAD_CDAE),
}
CONV_FAMILIES = [f for f in FAMILIES if f != "auxmnist"]

# Sharp criterion of part 1: the kernels' relative L2 error against float64 may be at most K_SHARP times the fp32 level of the tensor
# (_fp32_level) plus FLOOR.  Measured worst ratio of any gradient tensor on one MI355X: resconv 1.15, resconv_mlp 1.56, auxresconv 1.14,
# auxresconv_clip 1.97 (decode.dec.17.conv_0h.scale, a single number), conv 0.73, auxconv 1.20, auxmnist 0.78.  The fp32 oracle itself,
# on 12 further orders of the images, reaches 2.04x the level.  K_SHARP = 4: twice the worst measured ratio.  The col2im3 mutant named
# in test_vae_phase_recipe_batch_vs_float64 puts the residual-conv encoder's first-block gradients 5e-2 .. 4.5e-1 off.
K_SHARP = 4.0
FLOOR = 1e-7
FP32_ORDERS = 6


def _cfgs(family):
    mc, ctx, cc = FAMILIES[family]
    cc = O.CdaeCfg(cc.kind, cc.input_dim, ctx, cc.h_dim, cc.n_layers, cc.nonlin)
    return mc, cc


def _oracle_train_cfg(mc, nz, **kw):
    kw = dict(RES_RECIPE, **kw) if mc.kind in ("resconv", "auxresconv") else kw
    return O.TrainCfg(nz_cdae=nz, ctx_type="hidden1a" if mc.kind in O.AUX_KINDS else "lt0", **kw)


def _params(mc, cc):
    return O.init_params(O.model_param_spec(mc), 0, O.model_init_special(mc)), O.init_params(O.cdae_param_spec(cc), 1)


def _images(n, gen):
    return torch.bernoulli(torch.full((n, 784), 0.2), generator=gen)


def _vae_noise(mc, n, gen):
    """The VAE phase's draws (keys vae, vae_z, vctx_raw, vz0_raw of a step's noise), in the oracle's form."""
    full = O.draw_step_noise(mc, O.TrainCfg(nz_cdae=1), n, gen)
    return {k: v for k, v in full.items() if k.startswith("v")}


def _device_noise(mc, noise):
    """Oracle noise dict -> the engine's: an aux sampler's second draw sits beside the first, rows [eps0 | eps]."""
    out = {}
    for k, v in noise.items():
        if k.endswith("_z"):
            continue
        out[k] = torch.cat([v, noise[k + "_z"]], 1) if k + "_z" in noise else v
    return {k: v.cuda().contiguous() for k, v in out.items()}


def _cast(d, dtype):
    return {k: v.to(dtype) for k, v in d.items()}


def _engine(mc, cc, pm, pc, nb, **kw):
    model, cdae = build(mc, cc)
    model.load_state_dict(pm); cdae.load_state_dict(pc)
    model, cdae = model.to("cuda"), cdae.to("cuda")
    return model, cdae, net.ArdaeEngine(model, cdae, train_config(mc, NZ, **kw), batch_size=nb, graph=False)


def _profiled(fn):
    """Run fn() with the library's per-kernel profile on; -> {kernel name: launches}."""
    lib = L.lib()
    lib.ardae_profile_enable(1)
    try:
        fn()
        rep = L.profile_report(max_entries=256)
    finally:
        lib.ardae_profile_enable(0)
    return {e["name"]: e["calls"] for e in rep}


def _launches(prof, prefix):
    return sum(c for n, c in prof.items() if n.startswith(prefix))


def _split(flat, spec):
    out, off = {}, 0
    for n, shp in spec:
        k = int(np.prod(shp))
        out[n] = flat[off:off + k].reshape(shp)
        off += k
    return out


def _fp32_level(mc, cc, tc, pm, pc, x, noise, g64):
    """{gradient name: the rel. L2 error against float64 that fp32 arithmetic itself makes}.  One fp32 run is not a stable measure for
    small tensors: the scale and bias of the decoder's last, one-channel operators are single numbers, the result of a cancelling sum over
    100,352 rows, and their fp32 error is one draw of the rounding (merely permuting the 128 images changes the fp32 oracle's error of
    decode.dec.17.conv_0h.scale 20-fold).  So: the largest error of the fp32 oracle over FP32_ORDERS orders of the images (the
    gradients are sums over the images: permutations change only the rounding), and at least the median of all tensors' levels."""
    level = {n: 0.0 for n in g64}
    for k in range(FP32_ORDERS):
        perm = torch.randperm(x.size(0), generator=torch.Generator().manual_seed(k)) if k else torch.arange(x.size(0))
        g32 = O.vae_update_grads(mc, cc, tc, pm, pc, x[perm], {n: v[perm] for n, v in noise.items()})[4]
        for n in level:
            level[n] = max(level[n], rel_l2(g32[n], g64[n]))
    med = statistics.median(level.values())
    return {n: max(v, med) for n, v in level.items()}


def _zero_std_outputs(mc, tc, model, pm, x, noise):
    """encode(x, std=0) and the cDAE context of the device model next to the oracle's (with the parameters / images of pm / x's dtype)."""
    xd = x.cuda().float()
    if mc.clipped:           # the std = 0 calls are random draws: inject the unscaled eps0 the phase uses
        rc, rz = noise["vctx_raw"], noise["vz0_raw"]
        hid = model._hidden(xd, raw0=rc.float().cuda())
        z0 = model.forward_hidden(xd, std=0, nz=1, noise=rz.float().cuda())
        return [("z0", z0.reshape(x.size(0), -1), O.encode(mc, pm, x, O.zero_noise(mc, x.size(0), x, rz), 1).reshape(x.size(0), -1)),
                ("context", hid, O.cdae_context(mc, tc, pm, x, rc))]
    z0 = model.encode(xd, std=0)
    out = [("z0", z0.reshape(x.size(0), -1), O.encode(mc, pm, x, O.zero_noise(mc, x.size(0), x), 1).reshape(x.size(0), -1))]
    if mc.kind in O.AUX_KINDS:
        out.append(("context", model.encode.forward_hidden(xd, std=0), O.cdae_context(mc, tc, pm, x)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------ 1 + 2
@pytest.mark.parametrize("family", list(FAMILIES))
def test_vae_phase_recipe_batch_vs_float64(family):
    """The VAE phase (ivae_ardae.py:781-834, apply_update=False) at 128 images against the oracle in FLOAT64, run on the engine's own
    fp32 parameters, images and draws.

    Losses within 1e-4 relative (recon / prior 2e-5); encode(x, std=0), the cDAE context and decode_params (on 128 latents) within
    rel. L2 1e-5; every gradient tensor, by name (direction, scale and bias of each weight-normalised operator): rel. L2 below 2e-3
    (the backstop of the 4-image tests) AND at most K_SHARP x the fp32 oracle's own rel. L2 against float64 (_fp32_level) + FLOOR - an
    indexing or accumulation error confined to part of a large launch would stay far below 2e-3 in a tensor's norm but not below the
    fp32 level.

    Part 2: the phase runs under the library's kernel profile; the conv families must have launched the generic `linear_kernel<...>` and
    `wgrad_kernel` (not only `linear_small` / `wgrad_small_kernel`).  Seen on one MI355X: the residual-conv families 33 (37 for the
    clipped class) `linear_kernel<...>` launches over four instantiations and 10 `wgrad_kernel` batches; conv 8 and 1; auxconv 12 and 2.
    auxmnist (an MLP on 128 rows) stays on `linear_small` / `wgrad_small_kernel` and is not pinned.

    Sensitivity (shown once on a scratch build): with `col2im3_kernel` (resmodel.hip, residual-conv backward only) skipping the output
    elements past 1 << 20 - none at 4 images, where its largest launch is 50,176 elements; most of the 1,605,632 of the 28x28 blocks at
    128 - the 4-image suite passes, while this test fails for the four residual-conv families (first trunk block gradients off by
    5e-2 .. 4.5e-1) and so does test_engine_steps_exact_recipe_shape_vs_live_oracle for both residual-conv recipes."""
    mc, cc = _cfgs(family)
    tc = _oracle_train_cfg(mc, NZ)
    pm, pc = _params(mc, cc)
    gen = torch.Generator().manual_seed(101)
    x = _images(B, gen)
    noise = _vae_noise(mc, B, gen)
    model, cdae, eng = _engine(mc, cc, pm, pc, B)
    prof = _profiled(lambda: eng.vae_phase(x.cuda(), noise=_device_noise(mc, noise), apply_update=False))
    got = eng.stats()
    grads = _split(eng.grads_m.cpu(), O.model_param_spec(mc))

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    pm64, pc64, x64, n64 = _cast(pm, torch.float64), _cast(pc, torch.float64), x.double(), _cast(noise, torch.float64)
    l64, rec64, pri64, _, g64 = O.vae_update_grads(mc, cc, tc, pm64, pc64, x64, n64)
    assert rel(got["model_loss"], l64) < 1e-4, (got["model_loss"], float(l64))
    assert rel(got["recon"], rec64) < 2e-5 and rel(got["prior"], pri64) < 2e-5, (got, float(rec64), float(pri64))

    for what, dev, ref in _zero_std_outputs(mc, tc, model, pm64, x64, n64):
        assert rel_l2(dev, ref) < 1e-5, what
    z = torch.randn(B, mc.z_dim, generator=gen)
    (logit,) = model.decode_params(z.cuda())
    assert rel_l2(logit, O.decode(mc, pm64, z.double())[0]) < 1e-5

    level = _fp32_level(mc, cc, tc, pm, pc, x, noise, g64)
    bad, ratios = [], {}
    for n, _ in O.model_param_spec(mc):
        e_dev = rel_l2(grads[n], g64[n])
        ratios[n] = (e_dev / level[n], e_dev, level[n])
        if not (e_dev < 2e-3 and e_dev <= K_SHARP * level[n] + FLOOR):
            bad.append((n, e_dev, level[n]))
    worst = max(ratios.items(), key=lambda kv: kv[1][0])
    print(f"\n{family}: worst gradient ratio {worst[1][0]:.2f} ({worst[0]}: {worst[1][1]:.1e} vs fp32 level {worst[1][2]:.1e}); "
          f"fp32 levels {min(level.values()):.1e} .. {max(level.values()):.1e}; "
          f"largest error {max(r[1] for r in ratios.values()):.1e}; linear_kernel< x{_launches(prof, 'linear_kernel<')}, "
          f"wgrad_kernel x{prof.get('wgrad_kernel', 0)}, wgrad_small_kernel x{prof.get('wgrad_small_kernel', 0)}, "
          f"kernels {sorted(prof)}")
    assert not bad, bad

    if family in CONV_FAMILIES:
        assert _launches(prof, "linear_kernel<") > 0, sorted(prof)
        assert prof.get("wgrad_kernel", 0) > 0, sorted(prof)


def test_recipe_batch_runs_more_generic_kernels_than_fixture_batch():
    """The pin of part 2 against the fixtures' batch: the residual-conv VAE phase launches more `linear_kernel<...>` and `wgrad_kernel`
    at 128 images than at 4.  (Not zero at 4: the 28x28 blocks have 3136 rows there already, past the wgrad_small_kernel limit.)"""
    mc, cc = _cfgs("resconv")
    pm, pc = _params(mc, cc)
    counts = {}
    for nb in (4, B):
        gen = torch.Generator().manual_seed(7)
        x, noise = _images(nb, gen), _vae_noise(mc, nb, gen)
        _, _, eng = _engine(mc, cc, pm, pc, nb)
        prof = _profiled(lambda: eng.vae_phase(x.cuda(), noise=_device_noise(mc, noise), apply_update=False))
        counts[nb] = (_launches(prof, "linear_kernel<"), prof.get("wgrad_kernel", 0))
    print(f"\nresconv (linear_kernel<, wgrad_kernel) launches: 4 images {counts[4]}, 128 images {counts[B]}")
    assert counts[B][0] > counts[4][0] and counts[B][1] > counts[4][1], counts


# ------------------------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("family,k", [("resconv", 256), ("auxresconv", 256), ("auxresconv_clip", 256), ("conv", 1024), ("auxconv", 1024)])
def test_iwae_logprob_recipe_samples_vs_float64(family, k):
    """logprob (IWAE-k with the full-covariance Gaussian proposal) at the recipes' --iws-samples, 2 images, injected draws, against the
    oracle in float64: the sampler and the decoder run on 2k rows / images, through the generic kernels."""
    mc, cc = _cfgs(family)
    pm, _ = _params(mc, cc)
    model, _ = build(mc, cc)
    model.load_state_dict(pm)
    model = model.to("cuda")
    gen = torch.Generator().manual_seed(31)
    nb = 2
    x = _images(nb, gen)
    enc = torch.randn(nb, k, mc.noise_dim, generator=gen)
    if mc.kind in O.AUX_KINDS:
        enc = (enc, torch.randn(nb, k, mc.z_dim, generator=gen))
    prop = torch.randn(nb, k, mc.z_dim, generator=gen)
    dev_enc = tuple(e.cuda() for e in enc) if isinstance(enc, tuple) else enc.cuda()
    got = float(model.logprob(x.cuda(), sample_size=k, enc_noise=dev_enc, prop_noise=prop.cuda()))
    enc64 = tuple(e.double() for e in enc) if isinstance(enc, tuple) else enc.double()
    ref = float(O.iwae_logprob(mc, _cast(pm, torch.float64), x.double(), k, enc64, prop.double()))
    assert abs(got - ref) < 1e-4 * abs(ref), (got, ref)


# ------------------------------------------------------------------------------------------------------------------------------------ 4
# recipe: model, optimiser settings of the engine (TrainConfig) and the oracle, --num-cdae-updates, beta of step t
RECIPES = {
    "resconvct-res": ("resconv", 2, lambda t: 1.0),
    "auxresconvct": ("auxresconv", 2, lambda t: net.annealing_func(1e-4, 1.0, 50000, t)),    # --beta-init 0.0001 --beta-annealing 50000
    "mnist-conv": ("conv", 1, lambda t: 1.0),
}


@pytest.mark.parametrize("recipe", list(RECIPES))
def test_engine_steps_exact_recipe_shape_vs_live_oracle(recipe):
    """Three consecutive steps at the exact recipe shape (128 images x 625 samples = 80,000 cDAE rows) with the recipe's cDAE,
    --num-cdae-updates, optimisers / learning rates (RES_RECIPE for the residual-conv lines, Adam beta1 0.5 / RMSprop momentum 0.5
    for mnist-conv) and beta, against the live fp32 oracle, TEACHER-FORCED as in
    test_engine_trajectory_production_shapes_vs_live_oracle: before each step the oracle takes the engine's parameters and optimiser
    state from its checkpoints, then runs the step's cDAE updates (O.cdae_update_grads + rmsprop_step, once per update) and the VAE
    update on the same images and injected draws.  Losses 1e-4 relative, recon / prior 2e-5; the parameter updates with
    assert_update_close at step 0, afterwards rel. L2 below 5e-2 per step and a median below 5e-3.  Measured on one MI355X (worst loss
    error; worst update error of steps 1-2, model / cDAE): resconvct-res 4.4e-7; 8.8e-6 / 2.7e-6, auxresconvct 3.2e-6; 5.1e-6 / 2.4e-6,
    mnist-conv 1.0e-7; 2.8e-4 / 6.1e-4."""
    family, n_upd, beta_of = RECIPES[recipe]
    mc, cc = _cfgs(family)
    tc = _oracle_train_cfg(mc, NZ, num_cdae_updates=n_upd)
    pm, pc = _params(mc, cc)
    model, cdae, eng = _engine(mc, cc, pm, pc, B, num_cdae_updates=n_upd)
    mnames, cnames = [n for n, _ in O.model_param_spec(mc)], [n for n, _ in O.cdae_param_spec(cc)]
    nc = len(torch.cat([pc[n].reshape(-1) for n in cnames])) - (1 if cc.kind == "grad" else 0)     # grad: neglogprob.fc.bias is unused
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    gen = torch.Generator().manual_seed(47)
    worst, late = {"loss": 0.0, "recon_prior": 0.0}, []
    for t in range(3):
        beta = beta_of(t)
        xs = [_images(B, gen) for _ in range(n_upd)]
        xv = _images(B, gen)
        noises = [O.draw_step_noise(mc, tc, B, gen) for _ in range(n_upd)]
        mck, cck = eng.model_checkpoint(), eng.cdae_checkpoint()
        rm = {n: mck["state_dict"][n].detach().cpu().clone() for n in mnames}
        rc = {n: cck["state_dict"][n].detach().cpu().clone() for n in cnames}
        st_m = _oracle_opt_state(mck, mnames, ("exp_avg", "exp_avg_sq"))
        st_c = _oracle_opt_state(cck, cnames, ("square_avg", "momentum_buffer"))
        before_m, before_c = torch.cat([rm[n].reshape(-1) for n in mnames]), torch.cat([rc[n].reshape(-1) for n in cnames])
        dn = [_device_noise(mc, n) for n in noises]
        eng.step([x.cuda() for x in xs] if n_upd > 1 else xs[0].cuda(), xv.cuda(), noise=dn if n_upd > 1 else dn[0], beta=beta)
        got = eng.stats()
        for i in range(n_upd):
            closs, gc, _ = O.cdae_update_grads(mc, cc, tc, rm, rc, xs[i], noises[i])
            with torch.no_grad():
                O.rmsprop_step(rc, gc, st_c, tc.d_lr, tc.d_momentum)
        mloss, rec, pri, _, gm = O.vae_update_grads(mc, cc, tc, rm, rc, xv, noises[-1], beta=beta)
        with torch.no_grad():
            O.adam_ref_step(rm, gm, st_m, tc.m_lr, tc.m_beta1)
        for k, ref in (("cdae_loss", closs), ("model_loss", mloss)):
            assert rel(got[k], ref) < 1e-4, (t, k, got[k], float(ref))
            worst["loss"] = max(worst["loss"], rel(got[k], ref))
        for k, ref in (("recon", rec), ("prior", pri)):
            assert rel(got[k], ref) < 2e-5, (t, k, got[k], float(ref))
            worst["recon_prior"] = max(worst["recon_prior"], rel(got[k], ref))
        after_m, after_c = model.flat_params().cpu(), cdae.flat_params().cpu()[:nc]
        ref_m, ref_c = torch.cat([rm[n].reshape(-1) for n in mnames]), torch.cat([rc[n].reshape(-1) for n in cnames])[:nc]
        if t == 0:       # sign-like first optimiser steps (see assert_update_close)
            assert_update_close(after_c, before_c[:nc], ref_c, f"cdae update, step {t}")
            assert_update_close(after_m, before_m, ref_m, f"model update, step {t}")
        else:
            um, uc = rel_l2(after_m - before_m, ref_m - before_m), rel_l2(after_c - before_c[:nc], ref_c - before_c[:nc])
            late.append((um, uc))
            assert um < 5e-2 and uc < 5e-2, (t, um, uc)
    for k, name in ((0, "model"), (1, "cdae")):
        assert statistics.median(e[k] for e in late) < 5e-3, (name, late)
    print(f"\n{recipe}: worst loss error {worst['loss']:.1e}, recon / prior {worst['recon_prior']:.1e}, "
          f"update errors of steps 1-2 (model, cdae) {[(f'{a:.1e}', f'{b:.1e}') for a, b in late]}")


# ------------------------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("mc", [O.ModelCfg("mnist", 784, 100, 256, 32, 2, "softplus"), FAMILIES["conv"][0], FAMILIES["resconv"][0]],
                         ids=["mnist", "conv", "resconv"])
def test_model_vae_backward_grads_beta_accumulates(mc):
    """ardae_model_vae_backward(..., grads_beta) is documented as grads = grads_beta * grads + d/dparams (include/ardae_hip.h), while the
    engine and the module surface always pass 0: two forward + backward calls on the same inputs, with grads_beta 0 then 1, must leave
    twice the single gradient in every element (to the rounding of the one accumulating add), at 128 images."""
    model, _ = build(mc, O.CdaeCfg("grad", mc.z_dim, mc.z_dim, 32, 2))
    model.load_state_dict(O.init_params(O.model_param_spec(mc), 0, O.model_init_special(mc)))
    model = model.to("cuda")
    lib, d, st = L.lib(), model._desc, L.stream_ptr()
    gen = torch.Generator().manual_seed(5)
    x = _images(B, gen).cuda()
    noise = torch.randn(model._noise_numel(B, 1), generator=gen).cuda()
    dz = torch.randn(B, mc.z_dim, generator=gen).cuda()
    ws = model._ws(lib.ardae_model_workspace_floats(ctypes.byref(d), B, 1, 1))
    z, losses = torch.empty(B, mc.z_dim, device="cuda"), torch.empty(3, device="cuda")
    grads = torch.full_like(model._flat, float("nan"))
    once = None
    for gb in (0.0, 1.0):
        L.check(lib.ardae_model_vae_forward(ctypes.byref(d), L.ptr(model._flat), L.ptr(model._packed_weights()), L.ptr(x), L.ptr(noise), B, 1,
                                            1.0, L.ptr(ws), ws.numel(), L.ptr(z), L.ptr(losses), st), "ardae_model_vae_forward")
        L.check(lib.ardae_model_vae_backward(ctypes.byref(d), L.ptr(model._flat), L.ptr(model._packed_weights()), L.ptr(x), L.ptr(noise), B, 1,
                                             1.0, 1.0, L.ptr(dz), L.ptr(ws), ws.numel(), L.ptr(grads), gb, st), "ardae_model_vae_backward")
        torch.cuda.synchronize()
        if once is None:
            once = grads.clone()
            assert torch.isfinite(once).all() and bool((once != 0).any())
    twice = (2 * once).double()
    err = (grads.double() - twice).abs()
    bad = err > 2.0 ** -22 * twice.abs()
    spec = O.model_param_spec(mc)
    per = _split(bad.cpu(), spec)
    assert not bad.any(), [(n, int(per[n].sum())) for n, _ in spec if per[n].any()]
