"""Posterior diagnostics on the device: ardae_hist2d against np.histogram2d (equal counts), ardae_sample_logvar against float64,
the scaled draw against the plain draw, PosteriorDiagnostics against the module route, chunking, and ArdaeEngine.diagnostics.

Criteria: histogram counts are EQUAL to numpy's; log-variances meet the criterion of tests/test_iwae_eval_gpu.py (`_within`: at most 3 x the
max-abs error of the fp32 torch line it replaces, on the same device input, plus 1e-6 max|ref|); sampler outputs meet the bar of
tests/test_engine_gpu.py (rel_l2 < 1e-5)."""
import warnings

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O

pytestmark = pytest.mark.gpu

SAMPLER_BAR = 1e-5                                                              # tests/test_engine_gpu.py, every sampler comparison


def rel_l2(a, b):                                                               # tests/test_engine_gpu.py
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _within(got, glue, ref, what):                                              # tests/test_iwae_eval_gpu.py
    """got / glue: device fp32 results of the new path / the torch line it replaces; ref: float64 on the CPU."""
    ref = ref.double()
    e_new = float((got.double().cpu() - ref).abs().max())
    e_old = float((glue.double().cpu() - ref).abs().max())
    bound = 3 * e_old + 1e-6 * float(ref.abs().max())
    print(f"{what}: kernel {e_new:.3e}  torch line {e_old:.3e}  bound {bound:.3e}")
    assert e_new <= bound, (what, e_new, e_old, bound)


def _same_bits(a, b):
    return float((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).double().mean())


# ---- 1. ardae_hist2d == np.histogram2d --------------------------------------------------------------------------------------------------
RANGES = [(-4.0, 4.0, 128), (-6.0, 6.0, 128), (-3.0, 3.0, 5), (-6.0, 6.0, 100)]


def _hist(pts, n, row_stride, nslots, slot_stride, cx, cy, lo, hi, bins, counts=None):
    if counts is None:
        counts = torch.zeros(nslots, bins, bins, dtype=torch.int64, device="cuda")
    L.call("ardae_hist2d", pts, n, row_stride, nslots, slot_stride, cx, cy, lo, hi, bins, counts)
    return counts


def _numpy(x, y, lo, hi, bins):
    return np.histogram2d(x, y, range=[[lo, hi], [lo, hi]], bins=bins)[0].astype(np.int64)


def _normals(n, lo, hi, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, 2)) * (hi - lo) / 5).astype(np.float32)       # a few per cent fall outside the range


def _crafted(lo, hi, bins):
    """Every edge as float32 and its two float32 neighbours, the range's ends from both sides, -1e-30, +-inf, NaN - on either axis."""
    e = np.linspace(lo, hi, bins + 1).astype(np.float32)
    inf32 = np.float32(np.inf)
    v = np.concatenate([e, np.nextafter(e, -inf32), np.nextafter(e, inf32),
                        np.array([lo, hi, -lo, -hi, -1e-30, 1e-30, 0.0, -0.0, -1.8, 0.6, 1.8, -0.6, np.inf, -np.inf, np.nan], dtype=np.float32)])
    inside = np.full_like(v, np.float32(0.1))
    return np.concatenate([np.stack([v, v], 1), np.stack([v, inside], 1), np.stack([inside, v], 1), np.stack([v, v[::-1]], 1)])


_POINTS = {}


def _case(lo, hi, bins, case):
    """float32 points [n, 2] of a case, built once and left unchanged."""
    key = (lo, hi, bins, case)
    if key not in _POINTS:
        if case == "crafted":
            p = np.concatenate([_normals(1000, lo, hi, 1), _crafted(lo, hi, bins)])
        elif case == "contention":
            p = np.tile(np.array([[0.3, -1.1]], dtype=np.float32), (70001, 1))   # one bin takes every add
        else:
            p = _normals(case, lo, hi, case)
        _POINTS[key] = np.ascontiguousarray(p)
    return _POINTS[key]


@pytest.mark.parametrize("case", [1, 63, 64, 65, 1000, 70001, "crafted", "contention"])
@pytest.mark.parametrize("lo,hi,bins", RANGES)
def test_hist2d_equals_numpy(lo, hi, bins, case):
    p = _case(lo, hi, bins, case)
    want = _numpy(p[:, 0], p[:, 1], lo, hi, bins)
    got = _hist(torch.from_numpy(p).cuda(), len(p), 2, 1, 0, 0, 1, lo, hi, bins)[0].cpu().numpy()
    print(f"({lo}, {hi}, {bins}) {case}: {len(p)} points, {int(want.sum())} counted, {int((got != want).sum())} bins differ")
    assert np.array_equal(got, want)
    if case == "contention":
        assert got.max() == 70001 and (got != 0).sum() == 1


def test_hist2d_edges_that_are_no_float32_values():
    """(-3, 3, 5): the edges -0.6 and 1.8 are doubles just above the float32 values -0.6f and 1.8f, which round to them: compared in
    float32 both values would sit ON their edge and open the bin to its right; compared in double, as numpy does, they close the bin to its left."""
    e = np.linspace(-3, 3, 6)
    for v, k in ((-0.6, 2), (1.8, 4)):
        assert np.float32(e[k]) == np.float32(v) and np.float64(np.float32(v)) < e[k]
    p = np.array([[-0.6, 1.8], [1.8, -0.6]], dtype=np.float32)
    got = _hist(torch.from_numpy(p).cuda(), 2, 2, 1, 0, 0, 1, -3.0, 3.0, 5)[0].cpu().numpy()
    assert np.array_equal(got, _numpy(p[:, 0], p[:, 1], -3.0, 3.0, 5))
    assert got[1, 3] == 1 and got[3, 1] == 1 and got[2, 4] == 0 and got[4, 2] == 0


@pytest.mark.parametrize("lo,hi,bins", RANGES)
def test_hist2d_strided_layouts_and_slots(lo, hi, bins):
    n = 1000
    g = np.random.default_rng(7)
    # rows of 32 floats, the pair in columns 0 and 1 (a latent of z = 32), then in columns 5 and 2; NaN elsewhere would be dropped if read
    rows = (g.standard_normal((n, 32)) * (hi - lo) / 5).astype(np.float32)
    dev = torch.from_numpy(rows).cuda()
    assert np.array_equal(_hist(dev, n, 32, 1, 0, 0, 1, lo, hi, bins)[0].cpu().numpy(), _numpy(rows[:, 0], rows[:, 1], lo, hi, bins))
    assert np.array_equal(_hist(dev, n, 32, 1, 0, 5, 2, lo, hi, bins)[0].cpu().numpy(), _numpy(rows[:, 5], rows[:, 2], lo, hi, bins))
    # five slots side by side in a row, [n, 5, zd]: the stacked sampler call's output
    for zd in (2, 32):
        z = (g.standard_normal((n, 5, zd)) * (hi - lo) / 5 * np.array([1, .8, .5, .1, .01]).reshape(1, 5, 1)).astype(np.float32)
        guard = torch.full((7, bins, bins), 7, dtype=torch.int64, device="cuda")
        guard[1:6] = 0
        _hist(torch.from_numpy(z).cuda(), n, 5 * zd, 5, zd, 0, 1, lo, hi, bins, guard[1:6])
        got = guard.cpu().numpy()
        assert (got[0] == 7).all() and (got[6] == 7).all()                      # counts outside the addressed slots are untouched
        for s in range(5):
            assert np.array_equal(got[1 + s], _numpy(z[:, s, 0], z[:, s, 1], lo, hi, bins)), (zd, s)
        # slot-major blocks [5, n, zd]: what the per-slot sampler calls write
        zt = np.ascontiguousarray(z.transpose(1, 0, 2))
        got = _hist(torch.from_numpy(zt).cuda(), n, zd, 5, n * zd, 0, 1, lo, hi, bins).cpu().numpy()
        assert np.array_equal(got, guard[1:6].cpu().numpy())


@pytest.mark.parametrize("lo,hi,bins", RANGES)
def test_hist2d_adds_two_halves_like_one_whole(lo, hi, bins):
    p = _case(lo, hi, bins, 70001)
    dev = torch.from_numpy(p).cuda()
    whole = _hist(dev, len(p), 2, 1, 0, 0, 1, lo, hi, bins)
    h = 35001
    halves = _hist(dev, h, 2, 1, 0, 0, 1, lo, hi, bins)
    _hist(dev[h:], len(p) - h, 2, 1, 0, 0, 1, lo, hi, bins, halves)
    assert torch.equal(whole, halves)
    assert torch.equal(_hist(dev, len(p), 2, 1, 0, 0, 1, lo, hi, bins, whole.clone()), 2 * whole)       # it ADDS


# ---- 2. ardae_sample_logvar against float64 ---------------------------------------------------------------------------------------------
def _logvar(z):
    B, nz, zd = z.shape
    out = torch.full((B, zd), 123.0, device="cuda")
    L.call("ardae_sample_logvar", z, B, nz, zd, 1e-10, out)
    return out


def _torch_line(z):                                                             # ivae_ardae.py:957
    return torch.log(torch.var(z, dim=1) + 1e-10)


LOGVAR_SHAPES = [(1, 2, 1), (3, 64, 2), (5, 64, 32), (2, 7, 33), (4, 256, 64), (2, 4096, 2)]


@pytest.mark.parametrize("B,nz,zd", LOGVAR_SHAPES)
def test_sample_logvar_against_float64(B, nz, zd):
    g = torch.Generator().manual_seed(B * 1000 + nz + zd)
    spread = torch.logspace(-3, 1, zd).view(1, 1, zd)                           # columns with variances from 1e-6 to 1e2
    for name, z in (("unit", torch.randn(B, nz, zd, generator=g)), ("spread", torch.randn(B, nz, zd, generator=g) * spread),
                    ("mean 1e3 spread 1e-2", 1e3 + 1e-2 * torch.randn(B, nz, zd, generator=g))):
        z = z.float().cuda().contiguous()
        _within(_logvar(z), _torch_line(z), _torch_line(z.double().cpu()), f"({B}, {nz}, {zd}) {name}")


def test_sample_logvar_of_a_constant_column_is_log_eps():
    g = torch.Generator().manual_seed(3)
    for nz in (64, 7):
        z = torch.randn(3, nz, 4, generator=g)
        z[:, :, 1] = 0.37
        z[:, :, 3] = -1234.5678
        got = _logvar(z.cuda()).cpu()
        want = np.float32(np.log(np.float64(np.float32(1e-10))))                # the fp32 eps, its logarithm rounded once
        assert (got[:, [1, 3]].numpy() == want).all(), got
        assert bool(torch.isfinite(got).all())


def test_sample_logvar_of_one_row_is_nan():
    z = torch.randn(3, 1, 4).cuda()
    assert bool(torch.isnan(_logvar(z)).all())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                         # torch.var warns about the degrees of freedom, and gives NaN too
        assert bool(torch.isnan(_torch_line(z)).all())


@pytest.mark.parametrize("nz,zd", [(64, 32), (7, 33), (4096, 2)])
def test_sample_logvar_does_not_depend_on_the_launch(nz, zd):
    z = torch.randn(5, nz, zd, generator=torch.Generator().manual_seed(4)).cuda()
    batch = _logvar(z)
    for b in range(5):
        assert torch.equal(batch[b:b + 1], _logvar(z[b:b + 1].contiguous()))


# ---- 3. the scaled draw -----------------------------------------------------------------------------------------------------------------
SCALES = {1: [0.8], 5: [1.0, 0.8, 0.5, 0.1, 0.0]}


def _plain(n, seed, offset, first):
    t = torch.empty(n, device="cuda")
    L.call("ardae_philox_normal_at", t, n, seed, offset, None, first)
    return t


def _scaled(n, seed, offset, first, width, scale):
    t = torch.full((n,), float("nan"), device="cuda")
    L.call("ardae_philox_normal_scaled_at", t, n, seed, offset, None, first, width, scale.numel(), scale)
    return t


@pytest.mark.parametrize("width", [2, 34, 100])
@pytest.mark.parametrize("nslots", [1, 5])
def test_scaled_draw_is_the_plain_draw_times_the_slot_scale(nslots, width):
    seed, offset, R = 0xC0FFEE, net.rng.HOST_STREAM | 31, 7
    scale = torch.tensor(SCALES[nslots], device="cuda")
    n = R * nslots * width                                                      # 14 = 3 counters and a half: the ragged tail too
    for first in (0, 4 * width * nslots * 3):
        got = _scaled(n, seed, offset, first, width, scale).view(R, nslots, width)
        want = _plain(n, seed, offset, first).view(R, nslots, width) * scale.view(1, nslots, 1)
        assert torch.equal(got, want)
        if nslots == 5:
            assert bool((got[:, 4] == 0).all()) and not bool(torch.signbit(got[:, 4]).any())       # +0.0, whatever the draw's sign
            assert bool(torch.signbit(want[:, 4]).any())                                           # ... where the product has -0.0
            assert _same_bits(got[:, :4], want[:, :4]) == 1.0
    # a chunk's slice of the draw: rows [4, 8) of a 12-row draw
    whole = _scaled(12 * nslots * width, seed, offset, 0, width, scale).view(12, nslots, width)
    chunk = _scaled(4 * nslots * width, seed, offset, 4 * nslots * width, width, scale).view(4, nslots, width)
    assert _same_bits(whole[4:8], chunk) == 1.0
    unit = _scaled(n, seed, offset, 0, width, torch.ones(nslots, device="cuda"))
    assert _same_bits(unit, _plain(n, seed, offset, 0)) == 1.0


def test_scaled_draw_reads_the_step_state():
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    state[0] = 5                                                                # rng_offset
    scale = torch.tensor(SCALES[5], device="cuda")
    got = torch.empty(40, device="cuda")
    L.call("ardae_philox_normal_scaled_at", got, 40, 1, 2, state, 0, 2, 5, scale)
    assert torch.equal(got, _scaled(40, 1, 7, 0, 2, scale))


# ---- 4. the evaluator against the module route ------------------------------------------------------------------------------------------
MODELS = {"toy": O.ModelCfg("toy", 2, 10, 64, 2, 2, "relu"), "mnist": O.ModelCfg("mnist", 24, 10, 64, 8, 2, "softplus"),
          "auxmnist": O.ModelCfg("auxmnist", 24, 10, 48, 8, 2, "softplus"), "auxtoy": O.ModelCfg("auxtoy", 2, 2, 32, 2, 2, "tanh"),
          "conv": O.ModelCfg("conv", 784, 100, 800, 32, 1, "softplus"),                                      # conv_b4_nz8's widths
          "auxresconv_clip": O.ModelCfg("auxresconv", 784, 100, 450, 32, 1, "elu", clipped=True)}            # auxresconv_clip_b4_nz8's
_BUILT = {}


def _model(name):
    """The model on the device, built once per kind and left unchanged (as test_engine_gpu.py builds them)."""
    if name not in _BUILT:
        mc = MODELS[name]
        if mc.kind == "auxresconv":
            model = net.MNISTResConvAuxIPVAEClipped(input_height=28, input_channels=1, z_dim=mc.z_dim, c_dim=mc.h_dim, z0_dim=mc.noise_dim,
                                                    nonlinearity=mc.nonlin, do_center=mc.do_center)
        elif mc.kind == "conv":
            model = net.ConvIPVAE(input_height=28, input_channels=1, z_dim=mc.z_dim, noise_dim=mc.noise_dim, nonlinearity=mc.nonlin)
        elif mc.kind in ("auxtoy", "auxmnist"):
            model = (net.ToyAuxIPVAE if mc.kind == "auxtoy" else net.MNISTAuxIPVAE)(
                input_dim=mc.input_dim, noise_dim=mc.noise_dim, h_dim=mc.h_dim, num_hidden_layers=mc.n_layers, nonlinearity=mc.nonlin, enc_type="simple",
                z_dim=mc.z_dim, clip_z0_logvar=mc.clip_z0, clip_z_logvar=mc.clip_z)
        else:
            model = (net.MNISTIPVAE if mc.kind == "mnist" else net.ToyIPVAE)(
                input_dim=mc.input_dim, noise_dim=mc.noise_dim, h_dim=mc.h_dim, num_hidden_layers=mc.n_layers, nonlinearity=mc.nonlin, enc_type="concat",
                z_dim=mc.z_dim)
        model.load_state_dict(O.init_params(O.model_param_spec(mc), 0, O.model_init_special(mc)))
        _BUILT[name] = model.to("cuda")
    return _BUILT[name]


def _images(name, N, seed=0):
    mc, g = MODELS[name], torch.Generator().manual_seed(seed)
    if mc.kind in ("toy", "auxtoy"):
        return (2 * torch.randn(N, mc.input_dim, generator=g)).cuda()
    return torch.bernoulli(torch.full((N, mc.input_dim), 0.3), generator=g).cuda()


def _noise(model, N, S, seed=1):
    g = torch.Generator().manual_seed(seed)
    if model._kind in net.modules.AUX_KINDS:
        return (torch.randn(N, S, model.noise_dim, generator=g).cuda(), torch.randn(N, S, model.z_dim, generator=g).cuda())
    return torch.randn(N, S, model.noise_dim, generator=g).cuda()


def _slot(noise, s, scale=1.0):
    return tuple((n[:, s] * scale).contiguous() for n in noise) if isinstance(noise, tuple) else (noise[:, s] * scale).contiguous()


def _counts_equal_numpy_of(counts, latents, val, bins=128):
    z = latents.cpu().numpy()
    for s in range(z.shape[1]):
        assert np.array_equal(counts[s].cpu().numpy(), _numpy(z[:, s, 0], z[:, s, 1], -val, val, bins)), s


@pytest.mark.parametrize("name", ["toy", "mnist", "auxmnist", "auxtoy", "conv"])
def test_latents_are_the_module_routes_and_counts_are_numpys(name):
    model, N = _model(name), 12
    stds = net.diagnostics.STDS
    x, noise = _images(name, N), _noise(model, N, len(stds))
    pd = net.PosteriorDiagnostics(model)
    assert pd.stacked == (name != "auxtoy")
    counts, lat = pd.latent_histograms(x, noise=noise, return_latents=True)
    val = 4.0 if name in ("toy", "auxtoy") else 6.0
    assert counts.shape == (len(stds), 128, 128) and counts.dtype == torch.int64 and counts.is_cuda and lat.shape == (N, len(stds), model.z_dim)
    _counts_equal_numpy_of(counts, lat, val)
    for s, std in enumerate(stds):
        if std is None:
            want = model.forward_hidden(x, noise=_slot(noise, s))
        else:
            want = model.encode(x, std=std, noise=_slot(noise, s, float(std)))
        err = rel_l2(lat[:, s], want.view(N, -1))
        print(f"{name} std {std}: rel_l2 {err:.3e}, {100 * _same_bits(lat[:, s], want.view(N, -1)):.1f} % bit-identical")
        assert err < SAMPLER_BAR
    err = rel_l2(lat[:, -1], model.encode(x, std=0).view(N, -1))                # the std = 0 slot: the pass without noise
    print(f"{name} std 0 against encode(x, std=0): rel_l2 {err:.3e}")
    assert err < SAMPLER_BAR
    assert all(float((lat[:, s] - lat[:, -1]).abs().max()) > 0 for s in range(len(stds) - 1))       # the other levels carry their noise
    # another range, other bins: the reference's data range
    c2 = pd.latent_histograms(x, noise=noise, val=(-3, 3), bins=5)
    z = lat.cpu().numpy()
    assert all(np.array_equal(c2[s].cpu().numpy(), _numpy(z[:, s, 0], z[:, s, 1], -3, 3, 5)) for s in range(len(stds)))


def test_the_clipped_class_goes_slot_by_slot_with_its_raw_std0_pass():
    model, N, stds = _model("auxresconv_clip"), 12, (None, 0.0, 1)
    x, noise = _images("auxresconv_clip", N), _noise(_model("auxresconv_clip"), N, 3)
    pd = net.PosteriorDiagnostics(model)
    assert not pd.stacked
    with pytest.raises(NotImplementedError, match="std None, 1 or 0"):
        pd.latent_histograms(x)
    counts, lat = pd.latent_histograms(x, stds=stds, noise=noise, return_latents=True)
    _counts_equal_numpy_of(counts, lat, 6.0)
    want = [model.forward_hidden(x, noise=_slot(noise, 0)), model.forward_hidden(x, std=0, nz=1, noise=noise[0][:, 1].contiguous()),
            model.encode(x, std=1, noise=_slot(noise, 2))]
    for s in range(3):
        err = rel_l2(lat[:, s], want[s].view(N, -1))
        print(f"auxresconv_clip std {stds[s]}: rel_l2 {err:.3e}, {100 * _same_bits(lat[:, s], want[s].view(N, -1)):.1f} % bit-identical")
        assert err < SAMPLER_BAR
    own, _ = pd.latent_histograms(x, stds=stds, return_latents=True)
    assert own.sum(dim=(1, 2)).max() <= N


# ---- 5. chunking ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "mnist", "auxtoy"])
def test_result_does_not_depend_on_the_chunks(name):
    model, N, S = _model(name), 40, 5
    x = _images(name, N, seed=2)
    one = net.PosteriorDiagnostics(model)
    three = net.PosteriorDiagnostics(model, max_workspace_floats=one.latent_floats_per_chunk(16))
    assert one.plan_latent(N) == [(0, 40)] and three.plan_latent(N) == [(0, 16), (16, 32), (32, 40)]
    # the own draws: a chunk's launch writes the rows of the whole draw
    W, seed, offset = model._noise_width, 77, net.rng.HOST_STREAM | 0
    scale = torch.tensor([1.0, 0.8, 0.5, 0.1, 0.0], device="cuda")
    whole = _scaled(N * S * W, seed, offset, 0, W, scale).view(N, S, W)
    for i0, i1 in three.plan_latent(N):
        assert _same_bits(_scaled((i1 - i0) * S * W, seed, offset, i0 * S * W, W, scale).view(i1 - i0, S, W), whole[i0:i1]) == 1.0
    net.manual_seed(seed)
    ca, la = one.latent_histograms(x, return_latents=True)
    net.manual_seed(seed)
    cb, lb = three.latent_histograms(x, return_latents=True)
    err = rel_l2(lb, la)
    print(f"{name}: one chunk against three: rel_l2 {err:.3e}, {100 * _same_bits(la, lb):.1f} % bit-identical")
    assert err < SAMPLER_BAR
    # ... and they are the draw above, unscaled, injected
    plain = _plain(N * S * W, seed, offset, 0).view(N, S, W)
    inj = (plain[:, :, :model.noise_dim].contiguous(), plain[:, :, model.noise_dim:].contiguous()) if one.aux else plain
    _, li = one.latent_histograms(x, noise=inj, return_latents=True)
    assert rel_l2(li, la) < SAMPLER_BAR
    val = 4.0 if name in ("toy", "auxtoy") else 6.0
    for counts, lat in ((ca, la), (cb, lb)):
        _counts_equal_numpy_of(counts, lat, val)
        inside = ((lat[:, :, :2] >= -val) & (lat[:, :, :2] <= val)).all(dim=2).sum(dim=0)
        assert torch.equal(counts.sum(dim=(1, 2)), inside)                      # every slot: its in-range points, each once
    assert not torch.equal(la, one.latent_histograms(x, return_latents=True)[1])          # the next call draws anew
    with pytest.raises(ValueError, match="a chunk of 4 images"):
        net.PosteriorDiagnostics(model, max_workspace_floats=one.latent_floats_per_chunk(4) - 1).latent_histograms(x)


# ---- 6. data | reconstruction | generation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "auxtoy"])
def test_data_histograms(name):
    model, N = _model(name), 40
    x = _images(name, N, seed=3)
    one = net.PosteriorDiagnostics(model)
    three = net.PosteriorDiagnostics(model, max_workspace_floats=one.data_floats_per_chunk(16))
    assert len(three.plan_data(N)) == 3
    out = []
    for pd in (one, three):
        net.manual_seed(5)
        counts, recon, gen = pd.data_histograms(x, return_samples=True)
        assert counts.shape == (3, 128, 128) and counts.dtype == torch.int64 and recon.shape == gen.shape == x.shape
        for s, pts in enumerate((x, recon, gen)):
            p = pts.cpu().numpy()
            assert np.array_equal(counts[s].cpu().numpy(), _numpy(p[:, 0], p[:, 1], -6, 6, 128)), s
        assert bool(torch.isfinite(recon).all()) and bool(torch.isfinite(gen).all()) and not torch.equal(recon, gen)
        out.append((recon, gen))
    for what, a, b in zip(("recon", "gen"), *out):                              # the draws do not depend on the chunks
        print(f"{name} {what}: one chunk against three: rel_l2 {rel_l2(b, a):.3e}, {100 * _same_bits(a, b):.1f} % bit-identical")
        assert rel_l2(b, a) < SAMPLER_BAR
    c5 = one.data_histograms(x, val=3, bins=5)
    p = x.cpu().numpy()
    assert np.array_equal(c5[0].cpu().numpy(), _numpy(p[:, 0], p[:, 1], -3, 3, 5))
    with pytest.raises(NotImplementedError, match="Bernoulli"):
        net.PosteriorDiagnostics(_model("mnist")).data_histograms(_images("mnist", 8))


# ---- 7. log var q(z), run, the engine ---------------------------------------------------------------------------------------------------
def _hidden_noise(model, N, nz, seed=6):
    g = torch.Generator().manual_seed(seed)
    if model._kind == "auxtoy":
        q = model._q(nz)
        return (torch.randn(N, q, model.noise_dim, generator=g).cuda(), torch.randn(N, nz, model.z_dim, generator=g).cuda())
    return _noise(model, N, nz, seed)


@pytest.mark.parametrize("name", ["toy", "mnist", "auxmnist", "auxtoy"])
def test_logvar_qz_against_the_module_route(name):
    model, N, nz = _model(name), 12, 64
    x, noise = _images(name, N, seed=4), _hidden_noise(_model(name), N, nz)
    pd = net.PosteriorDiagnostics(model)
    got = pd.logvar_qz(x, nz, noise=noise)
    flat = tuple(n.reshape(-1, n.size(-1)) for n in noise) if isinstance(noise, tuple) else noise.reshape(N * nz, -1)
    latent = model.forward_hidden(x, nz=nz, noise=flat)                          # ivae_ardae.py:956
    line = _torch_line(latent)
    ref = _torch_line(latent.double().cpu())
    assert got.shape == (N, model.z_dim) and got.is_cuda
    _within(got, line, ref, f"{name} logvar_qz")
    _within(got.mean().view(1), line.mean().view(1), ref.mean().view(1), f"{name} mean")
    _within(got.median().view(1), line.median().view(1), ref.median().view(1), f"{name} median")
    # chunked, own draws: the same numbers
    small = net.PosteriorDiagnostics(model, max_workspace_floats=pd.logvar_floats_per_chunk(4))
    assert len(small.plan_logvar(N, nz)) == 3
    _within(small.logvar_qz(x, nz, noise=noise), line, ref, f"{name} logvar_qz in 3 chunks")
    # own draws: one Philox offset per block of the call, the same numbers whatever the chunks
    net.manual_seed(8)
    a = pd.logvar_qz(x, nz)
    net.manual_seed(8)
    b = small.logvar_qz(x, nz)
    blocks = [_plain(N * per_image, 8, net.rng.HOST_STREAM | i, 0) for i, per_image in enumerate(pd._logvar_blocks(nz))]
    if name == "auxtoy":
        own = (blocks[0].view(N, -1, model.noise_dim), blocks[1].view(N, nz, model.z_dim))
    elif pd.aux:
        rows = blocks[0].view(N, nz, model._noise_width)
        own = (rows[:, :, :model.noise_dim].contiguous(), rows[:, :, model.noise_dim:].contiguous())
    else:
        own = blocks[0].view(N, nz, model.noise_dim)
    assert torch.equal(a, pd.logvar_qz(x, nz, noise=own))
    flat = tuple(n.reshape(-1, n.size(-1)) for n in own) if isinstance(own, tuple) else own.reshape(N * nz, -1)
    latent = model.forward_hidden(x, nz=nz, noise=flat)
    _within(b, _torch_line(latent), _torch_line(latent.double().cpu()), f"{name} logvar_qz, own draws in 3 chunks")
    assert not torch.equal(a, pd.logvar_qz(x, nz))                              # the next call draws anew


@pytest.mark.parametrize("name", ["toy", "mnist"])
def test_run_is_the_three_parts_with_one_set_of_numbers(name):
    model = _model(name)
    x_all, x_batch = _images(name, 40, seed=9), _images(name, 8, seed=10)
    pd = net.PosteriorDiagnostics(model)
    net.manual_seed(21)
    out = pd.run(x_all, x_batch)
    net.manual_seed(21)
    latent = pd.latent_histograms(x_all)
    data = pd.data_histograms(x_all) if name == "toy" else None
    lv = pd.logvar_qz(x_batch)
    assert torch.equal(out["latent_counts"], latent) and out["latent_counts"].shape == (5, 128, 128)
    assert (out["data_counts"] is None) if data is None else torch.equal(out["data_counts"], data)
    assert isinstance(out["logvar_qz"], np.ndarray) and out["logvar_qz"].shape == (8, model.z_dim) and np.array_equal(out["logvar_qz"], lv.cpu().numpy())
    host = torch.from_numpy(out["logvar_qz"])
    assert out["logvar_qz_median"] == float(torch.median(host))                 # the lower middle value of an even count
    assert out["logvar_qz_median"] in out["logvar_qz"] and sorted(host.view(-1).tolist())[host.numel() // 2 - 1] == out["logvar_qz_median"]
    assert abs(out["logvar_qz_mean"] - float(host.double().mean())) <= 1e-6 * abs(float(host.double().mean())) + 1e-6
    assert out["enc/logvar_qz/mean/step"] == out["logvar_qz_mean"] and out["enc/logvar_qz/median/step"] == out["logvar_qz_median"]


def _engine(seed=11):
    mc, cc, B = MODELS["mnist"], O.CdaeCfg("grad", 8, 8, 64, 3), 8
    model = net.MNISTIPVAE(input_dim=mc.input_dim, noise_dim=mc.noise_dim, h_dim=mc.h_dim, num_hidden_layers=mc.n_layers, nonlinearity=mc.nonlin,
                           enc_type="concat", z_dim=mc.z_dim)
    cdae = net.MLPGradCARDAE(input_dim=cc.input_dim, context_dim=cc.context_dim, std=1., h_dim=cc.h_dim, num_hidden_layers=cc.n_layers,
                             nonlinearity=cc.nonlin, noise_type="gaussian", enc_ctx=True, enc_input=True)
    model.load_state_dict(O.init_params(O.model_param_spec(mc), 0, O.model_init_special(mc)))
    cdae.load_state_dict(O.init_params(O.cdae_param_spec(cc), 1))
    model, cdae = model.to("cuda"), cdae.to("cuda")
    net.manual_seed(seed)
    cfg = net.TrainConfig(nz_cdae=8, m_lr=1e-2, d_lr=1e-3, m_weight_avg="polyak", m_weight_avg_start=1, m_weight_avg_decay=0.5)
    return net.ArdaeEngine(model, cdae, cfg, batch_size=B), model, cdae


def test_engine_diagnostics_reads_the_live_weights_and_leaves_training_alone():
    g = torch.Generator().manual_seed(6)
    batches = [torch.bernoulli(torch.full((8, 24), 0.3), generator=g).cuda() for _ in range(8)]
    x_all = _images("mnist", 40, seed=12)
    runs = {}
    for with_diag in (True, False):
        eng, model, cdae = _engine()
        for i in range(3):                                                      # (the average leaves the live weights at its second step)
            eng.step(batches[2 * i], batches[2 * i + 1])
        if with_diag:
            before = model._flat.clone()
            st = net.rng.get_state()
            got = eng.diagnostics(x_all, batches[5])
            assert net.rng.get_state()["offset"] == st["offset"] + 2 and net.rng.get_state()["seed"] == st["seed"]     # host offsets, nothing else
            assert torch.equal(model._flat, before)
            net.manual_seed(st["seed"], st["offset"])
            want = net.PosteriorDiagnostics(model).run(x_all, batches[5])        # the live weights, not the averaged ones
            assert torch.equal(got["latent_counts"], want["latent_counts"]) and got["data_counts"] is None and want["data_counts"] is None
            assert np.array_equal(got["logvar_qz"], want["logvar_qz"])
            assert (got["logvar_qz_mean"], got["logvar_qz_median"]) == (want["logvar_qz_mean"], want["logvar_qz_median"])
            with eng.averaged_weights():
                avg = net.PosteriorDiagnostics(model).latent_histograms(x_all, stds=(0.0,), return_latents=True)[1]
            assert not torch.equal(avg, net.PosteriorDiagnostics(model).latent_histograms(x_all, stds=(0.0,), return_latents=True)[1])
            net.manual_seed(st["seed"], st["offset"])
            default = eng.diagnostics(x_all)                                    # x_batch: the first batch_size images
            assert default["logvar_qz"].shape == (8, 8) and int(default["latent_counts"].sum()) <= 5 * 40
            net.manual_seed(st["seed"], st["offset"])
        eng.step(batches[6], batches[7])
        runs[with_diag] = (model._flat.clone(), cdae._flat.clone(), eng.stats())
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1])      # bit-identical steps after it
    assert runs[True][2] == runs[False][2]
