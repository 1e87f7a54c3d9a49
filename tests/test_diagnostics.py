"""Posterior diagnostics, host side (no GPU): the chunk plans, the refusals of PosteriorDiagnostics and of its three ABI entries - all of
which come before anything is launched - and the exported names."""
import types

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import diagnostics as D


def _mnist(z_dim=8):
    return net.MNISTIPVAE(input_dim=24, noise_dim=10, h_dim=64, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=z_dim)


def _toy():
    return net.ToyIPVAE(input_dim=2, noise_dim=10, h_dim=64, num_hidden_layers=2, nonlinearity="relu", enc_type="concat", z_dim=2)


MODELS = {"mnist": _mnist, "toy": _toy, "auxmnist": lambda: net.MNISTAuxIPVAE(input_dim=24, noise_dim=10, h_dim=48, z_dim=8),
          "auxtoy": lambda: net.ToyAuxIPVAE()}


@pytest.fixture
def launches(monkeypatch):
    """Every launch goes through _lib._invoke and fetches the stream: record both (workspace queries are no launches)."""
    seen = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: seen.append("stream") or types.SimpleNamespace(cuda_stream=0))
    invoke = L._invoke
    monkeypatch.setattr(L, "_invoke", lambda name, args: (None if name.endswith("_floats") else seen.append(name)) or invoke(name, args))
    return seen


class OnDevice(torch.Tensor):
    """A stand-in for a device tensor: is_cuda is all the checks read of the device."""
    is_cuda = True


def dev(*shape):
    return torch.zeros(*shape).as_subclass(OnDevice)


# ---- chunk plans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(MODELS))
@pytest.mark.parametrize("N", [1, 7, 40, 20000])
def test_plans_cover_the_set_once_on_counter_boundaries_within_the_budget(kind, N):
    pd = net.PosteriorDiagnostics(MODELS[kind]())
    plans = [("latent", pd.plan_latent, pd.latent_floats_per_chunk), ("logvar", pd.plan_logvar, pd.logvar_floats_per_chunk)]
    if pd.gaussian:
        plans.append(("data", pd.plan_data, pd.data_floats_per_chunk))
    for what, plan, need in plans:
        pd.budget = 1 << 28
        assert plan(N) == [(0, N)], what                                        # the default budget takes 20000 images of these in one chunk
        pd.budget = need(8)                                                     # 8 images fit, 12 do not
        assert need(12) > pd.budget
        chunks = plan(N)
        assert chunks[0][0] == 0 and chunks[-1][1] == N and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])), what
        assert all(s % 4 == 0 and s < e for s, e in chunks), what               # a chunk starts on a Philox counter
        assert all(need(e - s) <= pd.budget for s, e in chunks) and max(e - s for s, e in chunks) <= 8, what
        assert len(chunks) == -(-N // max(e - s for s, e in chunks)), what
        pd.budget = need(4) - 1
        with pytest.raises(ValueError, match="a chunk of 4 images"):
            plan(N)


def test_roads_per_kind():
    road = {k: net.PosteriorDiagnostics(f()).stacked for k, f in MODELS.items()}
    assert road == {"mnist": True, "toy": True, "auxmnist": True, "auxtoy": False}
    assert D.STDS == (None, 0.8, 0.5, 0.1, 0.0) and D.MAX_BINS == 128
    pd = net.PosteriorDiagnostics(MODELS["auxtoy"]())
    assert pd._logvar_blocks(64) == (8 * 2, 64 * 2)
    with pytest.raises(ValueError, match="not a square"):
        pd.plan_logvar(8, nz=5)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refuses_bad_inputs_before_any_launch(launches):
    pd = net.PosteriorDiagnostics(_mnist())
    x = torch.zeros(5, 24)
    for call in (pd.latent_histograms, pd.logvar_qz, lambda t: pd.run(t, t), lambda t: pd.run(dev(5, 24), t)):
        with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):
            call(x)                                                             # a CPU tensor
        with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float64"):
            call(x.double())                                                    # the wrong dtype
        with pytest.raises(ValueError, match="must be contiguous"):
            call(torch.zeros(24, 5).t())
    with pytest.raises(TypeError, match="x_all: expected a float32 tensor on the GPU"):
        pd.latent_histograms(x.numpy())
    with pytest.raises(ValueError, match=r"x_all must be \[5, 1, 24\]"):
        pd.latent_histograms(dev(5, 25))
    for kw in (dict(bins=129), dict(bins=0)):
        with pytest.raises(ValueError, match="bins must be 1 .. 128"):
            pd.latent_histograms(dev(5, 24), **kw)
    for val in ((4.0, 4.0), (4.0, -4.0), 0.0, -1.0, float("inf"), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="finite lo < hi"):
            pd.latent_histograms(dev(5, 24), val=val)
    with pytest.raises(ValueError, match="stds is empty"):
        pd.latent_histograms(dev(5, 24), stds=())
    with pytest.raises(ValueError, match="nz must be >= 1"):
        pd.logvar_qz(dev(5, 24), nz=0)
    with pytest.raises(NotImplementedError, match="Bernoulli"):
        pd.data_histograms(dev(5, 24))
    toy = net.PosteriorDiagnostics(_toy())
    with pytest.raises(ValueError, match="bins must be 1 .. 128"):
        toy.data_histograms(dev(5, 2), bins=200)
    with pytest.raises(ValueError, match="finite lo < hi"):
        toy.data_histograms(dev(5, 2), val=(6, 6))
    with pytest.raises(TypeError, match="x_all: expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        toy.data_histograms(torch.zeros(5, 2))
    with pytest.raises(ValueError, match="z_dim >= 2"):
        net.PosteriorDiagnostics(_mnist(1)).latent_histograms(dev(5, 24))
    assert launches == []


def test_checks_injected_noise(launches):
    N, S = 5, 5
    pd = net.PosteriorDiagnostics(_mnist())
    assert pd._check_noise(None, N, S) is None
    assert pd._check_noise(dev(N, S, 10), N, S).shape == (N, S, 10)
    with pytest.raises(ValueError, match=r"noise must be \[5, 5, 10\]"):
        pd._check_noise(dev(N, S, 12), N, S)                                    # the wrong width
    with pytest.raises(ValueError, match=r"noise must be \[5, 5, 10\]"):
        pd._check_noise(dev(N, 4, 10), N, S)                                    # one slot short
    with pytest.raises(ValueError, match=r"noise must be \[5, 5, 10\]"):
        pd._check_noise(dev(N + 1, S, 10), N, S)
    with pytest.raises(TypeError, match="noise: expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        pd._check_noise(torch.zeros(N, S, 10), N, S)
    with pytest.raises(TypeError, match="noise: expected a float32 tensor on the GPU, got torch.float16"):
        pd._check_noise(dev(N, S, 10).half(), N, S)
    with pytest.raises(ValueError, match="noise must be contiguous"):
        pd._check_noise(dev(N, 10, S).transpose(1, 2), N, S)
    with pytest.raises(ValueError, match="is one tensor"):
        pd._check_noise((dev(N, S, 10), dev(N, S, 8)), N, S)
    aux = net.PosteriorDiagnostics(MODELS["auxmnist"]())
    assert [t.shape for t in aux._check_noise((dev(N, S, 10), dev(N, S, 8)), N, S)] == [(N, S, 10), (N, S, 8)]
    with pytest.raises(ValueError, match="is the pair"):
        aux._check_noise(dev(N, S, 18), N, S)
    with pytest.raises(ValueError, match=r"noise\[1\] must be \[5, 5, 8\]"):
        aux._check_noise((dev(N, S, 10), dev(N, S, 10)), N, S)
    toy = net.PosteriorDiagnostics(MODELS["auxtoy"]())
    with pytest.raises(ValueError, match=r"noise\[0\] must be \[5, 8, 2\]"):     # log var q(z) at nz = 64: 8 z0's x 8 z's
        toy._check_noise((dev(N, 64, 2), dev(N, 64, 2)), N, 64, rows0=8)
    # the whole call refuses them too, and before the sampler's workspace is touched
    with pytest.raises(ValueError, match=r"noise must be \[5, 5, 10\]"):
        pd.latent_histograms(dev(N, 24), noise=dev(N, S, 12))
    with pytest.raises(ValueError, match=r"noise must be \[5, 3, 10\]"):
        pd.latent_histograms(dev(N, 24), stds=(None, 0.5, 0.0), noise=dev(N, S, 10))
    assert launches == []


def test_the_clipped_class_takes_the_levels_its_module_takes():
    pd = types.SimpleNamespace(clipped=True, model=types.SimpleNamespace())
    assert D.PosteriorDiagnostics._scales(pd, (None, 1, 0.0)) == [1.0, 1.0, 0.0]
    with pytest.raises(NotImplementedError, match="std None, 1 or 0"):
        D.PosteriorDiagnostics._scales(pd, D.STDS)


def test_abi_entries_check_their_arguments_before_any_hip_call(launches):
    f32 = torch.zeros(8)

    def hist(pts=None, n=4, row_stride=2, nslots=1, slot_stride=0, col_x=0, col_y=1, lo=-4.0, hi=4.0, bins=128, counts=None):
        L.call("ardae_hist2d", pts, n, row_stride, nslots, slot_stride, col_x, col_y, lo, hi, bins, counts, None)

    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        hist(pts=f32)
    with pytest.raises(TypeError, match="expected a int64 tensor on the GPU, got torch.float32"):
        hist(counts=f32)
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        L.call("ardae_sample_logvar", f32, 1, 4, 2, 1e-10, None, None)
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float64"):
        L.call("ardae_philox_normal_scaled_at", None, 8, 0, 0, None, 0, 2, 1, f32.double(), None)
    assert launches == ["ardae_hist2d"] * 2 + ["ardae_sample_logvar", "ardae_philox_normal_scaled_at"]
    for bins in (0, 129, -1):
        with pytest.raises(ValueError, match=r"^ardae_hist2d: .*1 <= bins <= 128 \(got bins=%d\)" % bins):
            hist(bins=bins)
    for lo, hi in ((4.0, 4.0), (4.0, -4.0), (float("-inf"), 4.0), (-4.0, float("inf")), (float("nan"), 4.0)):
        with pytest.raises(ValueError, match="^ardae_hist2d: .*finite lo < hi"):
            hist(lo=lo, hi=hi)
    with pytest.raises(ValueError, match="^ardae_hist2d: .*n > 0"):
        hist(n=0)
    with pytest.raises(ValueError, match="^ardae_hist2d: .*nslots"):
        hist(nslots=0)
    with pytest.raises(ValueError, match="^ardae_hist2d: .*row_stride >= 1"):
        hist(row_stride=0)
    with pytest.raises(ValueError, match="^ardae_hist2d: .*col_x >= 0"):
        hist(col_x=-1)
    with pytest.raises(ValueError, match="^ardae_hist2d: .*must not be NULL"):
        hist()
    with pytest.raises(ValueError, match=r"^ardae_sample_logvar: .*nz >= 1, zd >= 1 \(got B=2, nz=0, zd=3\)"):
        L.call("ardae_sample_logvar", None, 2, 0, 3, 1e-10, None, None)
    with pytest.raises(ValueError, match="^ardae_sample_logvar: .*B > 0"):
        L.call("ardae_sample_logvar", None, 0, 4, 3, 1e-10, None, None)
    with pytest.raises(ValueError, match="^ardae_sample_logvar: .*eps"):
        L.call("ardae_sample_logvar", None, 2, 4, 3, -1.0, None, None)
    with pytest.raises(ValueError, match="^ardae_sample_logvar: .*must not be NULL"):
        L.call("ardae_sample_logvar", None, 2, 4, 3, 1e-10, None, None)
    for first in (1, 2, 3, 42):
        with pytest.raises(ValueError, match="^ardae_philox_normal_scaled_at: .*first_element must be a multiple of 4"):
            L.call("ardae_philox_normal_scaled_at", None, 8, 0, 0, None, first, 2, 1, None, None)
    for n, width, nslots in ((0, 2, 1), (8, 0, 1), (8, 2, 0)):
        with pytest.raises(ValueError, match="^ardae_philox_normal_scaled_at: .*n > 0, width >= 1, nslots >= 1"):
            L.call("ardae_philox_normal_scaled_at", None, n, 0, 0, None, 0, width, nslots, None, None)
    with pytest.raises(ValueError, match="^ardae_philox_normal_scaled_at: .*must not be NULL"):
        L.call("ardae_philox_normal_scaled_at", None, 8, 0, 0, None, 0, 2, 1, None, None)
    assert "stream" not in launches                                              # the stream was passed: none was fetched


def test_package_engine_and_header_expose_the_diagnostics():
    assert callable(net.PosteriorDiagnostics) and net.PosteriorDiagnostics is D.PosteriorDiagnostics
    assert hasattr(net.ArdaeEngine, "diagnostics")
    for m in ("latent_histograms", "data_histograms", "logvar_qz", "run"):
        assert callable(getattr(net.PosteriorDiagnostics, m))
    status = L.EXPORTS["ardae_iwae_reduce"][0]
    want = {"ardae_philox_normal_scaled_at": ["out", "n", "seed", "offset", "state", "first_element", "width", "nslots", "scale", "stream"],
            "ardae_sample_logvar": ["z", "B", "nz", "zd", "eps", "logvar", "stream"],
            "ardae_hist2d": ["pts", "n", "row_stride", "nslots", "slot_stride", "col_x", "col_y", "lo", "hi", "bins", "counts", "stream"]}
    for name, params in want.items():
        assert L.EXPORTS[name][0] is status and [p for p, _, _ in L.PROTOTYPES[name][1]] == params
        assert hasattr(L.lib(), name)                                           # ... and the built library has the symbol
    assert dict((p, pointee) for p, _, pointee in L.PROTOTYPES["ardae_hist2d"][1])["counts"] == "int64_t"
    assert L.CONSTANTS["ARDAE_ABI_VERSION"] == 1
    assert (D.TAG_MEAN, D.TAG_MEDIAN) == ("enc/logvar_qz/mean/step", "enc/logvar_qz/median/step")
