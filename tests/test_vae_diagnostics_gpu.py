"""GaussianDiagnostics, VaeEngine.diagnostics and PosteriorDiagnostics.final_pass on the device, at the smallest widths of each family.

Criteria: histogram counts are EQUAL to numpy's on the returned arrays; latents of the non-auxiliary kinds are BIT-EQUAL to model.encode's (the same
entry points on the same rows); MNISTAuxVAE / ToyAuxVAE latents meet TOL_LATENT (1e-5 relative L2, the bar tests/vae_gpu_checks.py sets and
tests/test_vae_aux_baseline_gpu.py holds ardae_vae_aux_iwae_draw's z to) against the float64 restatement; the two auxiliary conv kinds meet
2 x TOL_LATENT against model(x, eps)[2] - each of the two routes is held to TOL_LATENT against float64 by those files, so they differ by at most twice
that; results under different budgets are bit-equal."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import rng
from test_diagnostics_gpu import _images as ip_images
from test_diagnostics_gpu import _model as ip_model
from vae_gpu_checks import TOL_LATENT, np64, rel
from vae_restate import aux_logq_rows as logq_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"

BUILD = {"mnist": lambda: net.MNISTVAE(input_dim=24, h_dim=32, z_dim=8, nonlinearity="softplus", num_hidden_layers=2),
         "toy": lambda: net.ToyVAE(input_dim=2, h_dim=32, z_dim=2, nonlinearity="softplus", num_hidden_layers=1),
         "conv": lambda: net.MNISTConvVAE(z_dim=8), "resconv": lambda: net.MNISTResConvVAE(z_dim=8, c_dim=40),
         "auxmnist": lambda: net.MNISTAuxVAE(input_dim=24, noise_dim=10, h_dim=32, z_dim=8, nonlinearity="softplus", num_hidden_layers=2, clip_logvar="spm4"),
         "auxtoy": lambda: net.ToyAuxVAE(input_dim=2, noise_dim=2, h_dim=32, z_dim=2, nonlinearity="tanh", num_hidden_layers=1),
         "auxconv": lambda: net.MNISTConvAuxVAE(z0_dim=12, z_dim=8), "auxresconv": lambda: net.MNISTResConvAuxVAE(z0_dim=12, z_dim=8, c_dim=40)}
AUX_MLP = {"auxmnist": ("mnist", "softplus", "spm4"), "auxtoy": ("toy", "tanh", None)}      # logq_rows' cfg: family, activation, clip
_BUILT = {}


def _model(kind):
    """The model on the device, built once per kind and left unchanged."""
    if kind not in _BUILT:
        torch.manual_seed(sorted(BUILD).index(kind))
        _BUILT[kind] = BUILD[kind]().to(DEV)
    return _BUILT[kind]


def _images(kind, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind in ("toy", "auxtoy"):
        return (2 * torch.randn(N, 2, generator=g)).to(DEV)
    return torch.bernoulli(torch.full((N, _model(kind).input_dim), 0.3), generator=g).to(DEV)


def _numpy(p, lo, hi, bins):
    p = p.cpu().numpy()
    return np.histogram2d(p[:, 0], p[:, 1], range=[[lo, hi], [lo, hi]], bins=bins)[0].astype(np.int64)


def _plain(n, seed, offset):
    t = torch.empty(n, device=DEV)
    L.call("ardae_philox_normal_at", t, n, seed, offset, None, 0)
    return t


# ---- latents and counts, all eight classes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(BUILD))
def test_latents_are_the_models_and_counts_are_numpys(kind):
    m, N = _model(kind), 12
    x = _images(kind, N)
    eps = torch.randn(N, m._eps_width, generator=torch.Generator().manual_seed(1)).to(DEV)
    gd = net.GaussianDiagnostics(m)
    before = rng.get_state()
    counts, lat = gd.latent_histograms(x, eps=eps, return_latents=True)
    assert rng.get_state() == before                                            # an injected draw takes no offset
    val = 4.0 if kind in ("toy", "auxtoy") else 6.0
    assert counts.shape == (128, 128) and counts.dtype == torch.int64 and counts.is_cuda and lat.shape == (N, m.z_dim)
    assert np.array_equal(counts.cpu().numpy(), _numpy(lat, -val, val, 128))
    c5 = gd.latent_histograms(x, eps=eps, val=(-3, 3), bins=5)
    assert np.array_equal(c5.cpu().numpy(), _numpy(lat, -3, 3, 5))
    if not gd.aux:
        assert torch.equal(lat, m.encode(x, eps=eps)[0])                        # the same entry points on the same rows
    elif kind in AUX_MLP:
        want, _ = logq_rows({n: np64(v) for n, v in m.named_parameters()}, AUX_MLP[kind], np64(x), np64(eps).reshape(N, 1, -1))
        err = rel(np64(lat), want)
        print(f"{kind}: latents against float64: rel L2 {err:.3e}")
        assert err <= TOL_LATENT
    else:
        err = rel(np64(lat), np64(m(x, eps=eps)[2]))
        print(f"{kind}: latents against model(x, eps)[2]: rel L2 {err:.3e}")
        assert err <= 2 * TOL_LATENT


# ---- budget independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,lengths,nchunks", [("mnist", 200, (100, 48), (2, 5)), ("auxmnist", 200, (100, 48), (2, 5)), ("conv", 250, (128, 64), (2, 4))])
def test_result_does_not_depend_on_the_budget(kind, N, lengths, nchunks):
    m = _model(kind)
    x = _images(kind, N, seed=2)
    one = net.GaussianDiagnostics(m)
    assert one.plan(N) == [(0, N)]
    net.manual_seed(77)
    ca, la = one.latent_histograms(x, return_latents=True)
    assert rng.get_state()["offset"] == (2 if one.aux else 1)                   # one offset per draw and per call
    for c, n in zip(lengths, nchunks):
        small = net.GaussianDiagnostics(m, max_workspace_floats=one.floats_per_chunk(c))
        plan = small.plan(N)
        assert len(plan) == n and all(s % (one.group or 4) == 0 for s, _ in plan)
        net.manual_seed(77)
        cb, lb = small.latent_histograms(x, return_latents=True)
        assert torch.equal(la, lb) and torch.equal(ca, cb)                      # to the bit
    assert np.array_equal(ca.cpu().numpy(), _numpy(la, -6, 6, 128)) and int(ca.sum()) <= N
    net.manual_seed(78)
    assert not torch.equal(la, one.latent_histograms(x, return_latents=True)[1])
    if kind == "mnist":                                                         # the draw is the documented one: element i of the call's offset
        e = _plain(N * m.z_dim, 77, rng.HOST_STREAM | 0).view(N, m.z_dim)
        assert torch.equal(la, one.latent_histograms(x, eps=e, return_latents=True)[1])
    if kind == "auxmnist":                                                      # eps0 and eps: elements of offset0 and offset1, rows [eps0 | eps]
        e = torch.cat([_plain(N * m.noise_dim, 77, rng.HOST_STREAM | 0).view(N, -1), _plain(N * m.z_dim, 77, rng.HOST_STREAM | 1).view(N, -1)], 1)
        assert torch.equal(la, one.latent_histograms(x, eps=e.contiguous(), return_latents=True)[1])


# ---- data | reconstruction | generation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["toy", "auxtoy"])
def test_data_histograms(kind):
    m, N, D, zd = _model(kind), 40, 2, 2
    x = _images(kind, N, seed=3)
    one = net.GaussianDiagnostics(m)
    three = net.GaussianDiagnostics(m, max_workspace_floats=one.floats_per_chunk(16, True))
    assert one.plan(N, True) == [(0, N)] and len(three.plan(N, True)) == 3
    n_lat = 2 if one.aux else 1
    out = []
    for gd in (one, three):
        net.manual_seed(5)
        counts, recon, gen, lat = gd.data_histograms(x, return_samples=True)
        assert rng.get_state()["offset"] == n_lat + 3
        assert counts.shape == (3, 128, 128) and counts.dtype == torch.int64 and recon.shape == gen.shape == x.shape and lat.shape == (N, zd)
        for s, pts in enumerate((x, recon, gen)):                               # slot 0 is the data
            assert np.array_equal(counts[s].cpu().numpy(), _numpy(pts, -6, 6, 128)), s
        out.append((counts, recon, gen, lat))
    assert all(torch.equal(a, b) for a, b in zip(*out))                         # the budget does not show
    counts, recon, gen, lat = out[0]
    # the reconstruction decodes the latent of the same walk on the documented draw; the generation decodes z ~ N(0, I)
    assert torch.equal(recon, m._decoder_sample(lat, _plain(N * D, 5, rng.HOST_STREAM | n_lat).view(N, D))[0])
    zg = _plain(N * zd, 5, rng.HOST_STREAM | (n_lat + 1)).view(N, zd)
    assert torch.equal(gen, m._decoder_sample(zg, _plain(N * D, 5, rng.HOST_STREAM | (n_lat + 2)).view(N, D))[0])
    # ... and that latent is the one latent_histograms bins under the same rng state; run makes both tables in one walk
    net.manual_seed(5)
    lc, l2 = one.latent_histograms(x, return_latents=True)
    assert torch.equal(l2, lat) and np.array_equal(lc.cpu().numpy(), _numpy(lat, -4, 4, 128))
    net.manual_seed(5)
    both = one.run(x)
    assert sorted(both) == ["data_counts", "latent_counts"] and torch.equal(both["latent_counts"], lc) and torch.equal(both["data_counts"], counts)
    c5 = one.data_histograms(x, val=3, bins=5)
    assert np.array_equal(c5[0].cpu().numpy(), _numpy(x, -3, 3, 5))
    with pytest.raises(NotImplementedError, match="Bernoulli"):
        net.GaussianDiagnostics(_model("mnist")).data_histograms(_images("mnist", 8))
    assert net.GaussianDiagnostics(_model("mnist")).run(_images("mnist", 8))["data_counts"] is None


# ---- the last block: 256 bins -----------------------------------------------------------------------------------------------------------
def test_final_pass_of_a_gaussian_baseline():
    m, N = _model("toy"), 1000
    x = _images("toy", N, seed=4)
    gd = net.GaussianDiagnostics(m)
    net.manual_seed(9)
    out = gd.final_pass(x, return_arrays=True)
    assert out["latent_counts"].shape == (256, 256) and out["data_counts"].shape == (3, 256, 256)
    assert np.array_equal(out["latent_counts"].cpu().numpy(), _numpy(out["latents"], -4, 4, 256))
    for s, pts in enumerate((x, out["recon"], out["gen"])):
        assert np.array_equal(out["data_counts"][s].cpu().numpy(), _numpy(pts, -6, 6, 256)), s
    assert 0 < int(out["latent_counts"].sum()) <= N
    net.manual_seed(9)
    plain = gd.final_pass(x)
    assert sorted(plain) == ["data_counts", "latent_counts"] and all(torch.equal(plain[k], out[k]) for k in plain)
    # (-4, 4) at 256 and at 128 bins: every second edge of the one is an edge of the other, exactly (steps 2^-5 and 2^-4) - the small table, which
    # goes through ardae_hist2d, is the wide one's 2 x 2 sums
    net.manual_seed(9)
    assert torch.equal(gd.final_pass(x, bins=128)["latent_counts"], plain["latent_counts"].view(128, 2, 128, 2).sum((1, 3)))
    image = net.GaussianDiagnostics(_model("mnist")).final_pass(_images("mnist", 12), return_arrays=True)      # any kind; latent val 4 here too
    assert image["data_counts"] is None and np.array_equal(image["latent_counts"].cpu().numpy(), _numpy(image["latents"], -4, 4, 256))


def test_final_pass_of_the_implicit_models():
    m, N = ip_model("toy"), 1000
    x = ip_images("toy", N, seed=5)
    pd = net.PosteriorDiagnostics(m)
    out = pd.final_pass(x, return_arrays=True)
    assert out["latent_counts"].shape == (5, 256, 256) and out["data_counts"].shape == (3, 256, 256) and out["latents"].shape == (N, 5, 2)
    for s in range(5):
        assert np.array_equal(out["latent_counts"][s].cpu().numpy(), _numpy(out["latents"][:, s], -4, 4, 256)), s
    for s, pts in enumerate((x, out["recon"], out["gen"])):
        assert np.array_equal(out["data_counts"][s].cpu().numpy(), _numpy(pts, -6, 6, 256)), s
    assert sorted(pd.final_pass(x)) == ["data_counts", "latent_counts"]
    # the clipped class takes its three levels
    clipped, xc = net.PosteriorDiagnostics(ip_model("auxresconv_clip")), ip_images("auxresconv_clip", 12)
    out = clipped.final_pass(xc, return_arrays=True)
    assert out["latent_counts"].shape == (3, 256, 256) and out["data_counts"] is None and out["latents"].shape == (12, 3, 32)
    for s in range(3):
        assert np.array_equal(out["latent_counts"][s].cpu().numpy(), _numpy(out["latents"][:, s], -4, 4, 256)), s


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------
def _engine():
    torch.manual_seed(3)
    m = BUILD["mnist"]().to(DEV)
    net.manual_seed(11)
    cfg = net.VaeConfig(lr=1e-2, weight_avg="polyak", weight_avg_start=1, weight_avg_decay=0.5, beta_init=0.1, beta_annealing=4)
    return net.VaeEngine(m, cfg, batch_size=8), m


def test_engine_diagnostics_reads_the_live_weights_and_leaves_training_alone():
    g = torch.Generator().manual_seed(6)
    batches = [torch.bernoulli(torch.full((8, 24), 0.3), generator=g).to(DEV) for _ in range(5)]
    x_all = _images("mnist", 40, seed=12)
    runs = {}
    for with_diag in (True, False):
        eng, m = _engine()
        for i in range(3):                                                      # the third call captures the step
            eng.step(batches[i])
        if with_diag:
            flat, state, st = m._flat.clone(), eng.state.clone(), rng.get_state()
            got = eng.diagnostics(x_all)
            assert rng.get_state() == {"seed": st["seed"], "offset": st["offset"] + 1}      # a host offset, nothing else
            assert torch.equal(m._flat, flat) and torch.equal(eng.state, state)             # the in-step Philox base among it
            net.manual_seed(st["seed"], st["offset"])
            want = net.GaussianDiagnostics(m).run(x_all)                        # the live weights, not the averaged ones
            assert torch.equal(got["latent_counts"], want["latent_counts"]) and got["data_counts"] is None and want["data_counts"] is None
            assert got["latent_counts"].shape == (128, 128) and 0 < int(got["latent_counts"].sum()) <= 40
            with eng.averaged_weights():
                with pytest.raises(RuntimeError, match="while the averaged weights are in"):
                    eng.diagnostics(x_all)
            assert torch.equal(m._flat, flat)
        for i in (3, 4):
            eng.step(batches[i])
        runs[with_diag] = (m._flat.clone(), eng.state.clone(), eng.losses.clone())
    assert all(torch.equal(a, b) for a, b in zip(runs[True], runs[False]))      # bit-identical steps after it
