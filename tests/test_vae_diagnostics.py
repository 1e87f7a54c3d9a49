"""Diagnostics of the Gaussian baselines and the wide histogram, host side (no GPU): the chunk plans, the refusals of GaussianDiagnostics, of
PosteriorDiagnostics.final_pass and of ardae_hist2d_wide - all of which come before anything is launched - and the exported names."""
import types

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import diagnostics as D
from ardae_amd import vae_diagnostics as V

MODELS = {"mnist": lambda: net.MNISTVAE(input_dim=24, h_dim=32, z_dim=8), "toy": lambda: net.ToyVAE(input_dim=2, h_dim=32, z_dim=2),
          "auxmnist": lambda: net.MNISTAuxVAE(input_dim=24, noise_dim=10, h_dim=32, z_dim=8),
          "auxtoy": lambda: net.ToyAuxVAE(input_dim=2, noise_dim=2, h_dim=32, z_dim=2),
          "conv": lambda: net.MNISTConvVAE(z_dim=8), "resconv": lambda: net.MNISTResConvVAE(z_dim=8, c_dim=40),
          "auxconv": lambda: net.MNISTConvAuxVAE(z0_dim=12, z_dim=8), "auxresconv": lambda: net.MNISTResConvAuxVAE(z0_dim=12, z_dim=8, c_dim=40)}


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
@pytest.mark.parametrize("N", [1, 7, 200, 20000])
def test_plans_cover_the_set_once_on_group_boundaries_within_the_budget(kind, N):
    gd = net.GaussianDiagnostics(MODELS[kind]())
    G = gd.group or 4
    assert gd.group == (None if kind in ("mnist", "toy", "auxmnist", "auxtoy") else 64) and gd.aux == kind.startswith("aux")
    for data in ((False, True) if gd.gaussian else (False,)):
        need = lambda c: gd.floats_per_chunk(c, data)                           # noqa: E731
        gd.budget = 1 << 28
        if not gd.group:
            assert gd.plan(N, data) == [(0, N)]                                  # the default budget takes 20000 images of the MLP kinds in one chunk
        gd.budget = need(2 * G)                                                 # two groups fit, three do not
        assert need(3 * G) > gd.budget
        chunks = gd.plan(N, data)
        assert chunks[0][0] == 0 and chunks[-1][1] == N and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(s % G == 0 and s < e for s, e in chunks)                     # a chunk starts on a Philox counter, or on a whole group
        assert all(need(e - s) <= gd.budget for s, e in chunks) and max(e - s for s, e in chunks) <= 2 * G
        if N == 20000:
            assert len(chunks) == -(-N // (2 * G))
        gd.budget = need(G) - 1
        if gd.group and N > G:
            with pytest.raises(ValueError, match=f"GaussianDiagnostics: the budget of {gd.budget} floats is below one group of 64 images"):
                gd.plan(N, data)
        elif not gd.group:
            with pytest.raises(ValueError, match="a chunk of 4 images"):
                gd.plan(N, data)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refuses_bad_inputs_before_any_launch(launches):
    gd = net.GaussianDiagnostics(MODELS["mnist"]())
    x = torch.zeros(5, 24)
    for call in (gd.latent_histograms, gd.run, gd.final_pass):
        with pytest.raises(TypeError, match="GaussianDiagnostics: x_all: expected a float32 tensor on the GPU, got torch.float32 on cpu"):
            call(x)                                                             # a CPU tensor
        with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float64"):
            call(x.double())                                                    # the wrong dtype
        with pytest.raises(ValueError, match="must be contiguous"):
            call(torch.zeros(24, 5).t())
        with pytest.raises(ValueError, match=r"x_all must be \[5, 1, 24\]"):
            call(dev(5, 25))
    with pytest.raises(TypeError, match="x_all: expected a float32 tensor on the GPU"):
        gd.latent_histograms(x.numpy())
    for bins in (513, 0, -1):
        with pytest.raises(ValueError, match="GaussianDiagnostics: bins must be 1 .. 512"):
            gd.latent_histograms(dev(5, 24), bins=bins)
        with pytest.raises(ValueError, match="bins must be 1 .. 512"):
            gd.final_pass(dev(5, 24), bins=bins)
    for val in ((4.0, 4.0), (4.0, -4.0), 0.0, -1.0, float("inf"), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="GaussianDiagnostics: the range needs finite lo < hi"):
            gd.latent_histograms(dev(5, 24), val=val)
    with pytest.raises(NotImplementedError, match="Bernoulli"):
        gd.data_histograms(dev(5, 24))
    for eps in (dev(5, 9), dev(4, 8), dev(5, 2, 8)):
        with pytest.raises(ValueError, match=r"eps must be \[5, 1, 8\]"):
            gd.latent_histograms(dev(5, 24), eps=eps)
    with pytest.raises(TypeError, match="eps: expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        gd.latent_histograms(dev(5, 24), eps=torch.zeros(5, 8))
    with pytest.raises(ValueError, match="eps must be contiguous"):
        gd.latent_histograms(dev(5, 24), eps=dev(8, 5).t())
    with pytest.raises(ValueError, match="z_dim >= 2"):
        net.GaussianDiagnostics(net.MNISTVAE(input_dim=24, h_dim=32, z_dim=1)).latent_histograms(dev(5, 24))
    with pytest.raises(ValueError, match=r"eps must be \[5, 1, 18\]"):          # the auxiliary-variable kinds: rows [eps0 | eps]
        net.GaussianDiagnostics(MODELS["auxmnist"]()).latent_histograms(dev(5, 24), eps=dev(5, 8))
    toy = net.GaussianDiagnostics(MODELS["toy"]())
    with pytest.raises(ValueError, match="bins must be 1 .. 512"):
        toy.data_histograms(dev(5, 2), bins=600)
    with pytest.raises(ValueError, match="finite lo < hi"):
        toy.data_histograms(dev(5, 2), val=(6, 6))
    with pytest.raises(TypeError, match="x_all: expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        toy.data_histograms(torch.zeros(5, 2))
    with pytest.raises(ValueError, match="input_dim >= 2"):
        net.GaussianDiagnostics(net.ToyVAE(input_dim=1, h_dim=32, z_dim=2)).data_histograms(dev(5, 1))
    # the budget: below 4 images, and below one group of a conv kind
    small = net.GaussianDiagnostics(MODELS["toy"](), max_workspace_floats=toy.floats_per_chunk(4, True) - 1)
    for call in (small.data_histograms, small.run, small.final_pass):
        with pytest.raises(ValueError, match="a chunk of 4 images"):
            call(dev(40, 2))
    conv = net.GaussianDiagnostics(MODELS["conv"]())
    conv.budget = conv.floats_per_chunk(64) - 1
    with pytest.raises(ValueError, match="is below one group of 64 images"):
        conv.latent_histograms(dev(200, 784))
    assert launches == []


def test_takes_the_gaussian_classes_only():
    for kind, make in MODELS.items():
        gd = net.GaussianDiagnostics(make())
        assert gd.gaussian == (kind in ("toy", "auxtoy")) and gd.sd == (gd.model.noise_dim if gd.aux else gd.model.z_dim)
    for other in (net.MNISTIPVAE(input_dim=24, noise_dim=10, h_dim=64, z_dim=8), torch.nn.Linear(2, 2)):
        with pytest.raises(TypeError, match="PosteriorDiagnostics"):
            net.GaussianDiagnostics(other)
    with pytest.raises(NotImplementedError, match="z_dim 129 > 128"):
        net.GaussianDiagnostics(net.MNISTAuxVAE(input_dim=24, noise_dim=10, h_dim=32, z_dim=129))


def test_final_pass_of_the_implicit_models_refuses_before_any_launch(launches):
    pd = net.PosteriorDiagnostics(net.MNISTIPVAE(input_dim=24, noise_dim=10, h_dim=64, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat",
                                                 z_dim=8))
    for bins in (513, 0):
        with pytest.raises(ValueError, match="PosteriorDiagnostics: bins must be 1 .. 512"):
            pd.final_pass(dev(5, 24), bins=bins)
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        pd.final_pass(torch.zeros(5, 24))
    with pytest.raises(ValueError, match="bins must be 1 .. 128"):              # the two existing methods keep their cap
        pd.latent_histograms(dev(5, 24), bins=256)
    assert (D.MAX_BINS, D.MAX_BINS_WIDE) == (128, 512)
    assert launches == []


def test_the_dispatch_sends_small_tables_to_the_lds_kernel(monkeypatch):
    seen = []
    monkeypatch.setattr(L, "call", lambda name, *a: seen.append((name, a[9])))
    for bins in (1, 128, 129, 256, 512):
        D.hist2d(None, 4, 2, 1, 0, 0, 1, -4.0, 4.0, bins, None)
    D.hist2d_lds(None, 4, 2, 1, 0, 0, 1, -4.0, 4.0, 128, None)
    assert seen == [("ardae_hist2d", 1), ("ardae_hist2d", 128), ("ardae_hist2d_wide", 129), ("ardae_hist2d_wide", 256), ("ardae_hist2d_wide", 512),
                    ("ardae_hist2d", 128)]


def test_engine_diagnostics_is_refused_while_the_averaged_weights_are_in():
    eng = types.SimpleNamespace(_avg_swap=True, _require_trained=lambda what: net.VaeEngine._require_trained(eng, what))
    with pytest.raises(RuntimeError, match=r"VaeEngine.diagnostics\(\) while the averaged weights are in"):
        net.VaeEngine.diagnostics(eng, dev(8, 24))


# ---- the ABI entry ----------------------------------------------------------------------------------------------------------------------
def test_hist2d_wide_checks_its_arguments_before_any_hip_call(launches):
    one = 64                                                                    # any non-null address: validation fails before it is dereferenced

    def hist(pts=one, n=4, row_stride=2, nslots=1, slot_stride=0, col_x=0, col_y=1, lo=-4.0, hi=4.0, bins=256, counts=one):
        L.call("ardae_hist2d_wide", pts, n, row_stride, nslots, slot_stride, col_x, col_y, lo, hi, bins, counts, None)

    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        hist(pts=torch.zeros(8))
    with pytest.raises(TypeError, match="expected a int64 tensor on the GPU, got torch.float32"):
        hist(counts=torch.zeros(8))
    for bins in (0, 513, -1):
        with pytest.raises(ValueError, match=r"^ardae_hist2d_wide: .*hist2d_wide: need 1 <= bins <= 512 \(got bins=%d\)$" % bins):
            hist(bins=bins)
    for lo, hi in ((4.0, 4.0), (4.0, -4.0), (float("-inf"), 4.0), (-4.0, float("inf")), (float("nan"), 4.0)):
        with pytest.raises(ValueError, match="^ardae_hist2d_wide: .*hist2d_wide: need finite lo < hi"):
            hist(lo=lo, hi=hi)
    with pytest.raises(ValueError, match="^ardae_hist2d_wide: .*n > 0"):
        hist(n=0)
    for nslots in (0, 65536):
        with pytest.raises(ValueError, match="^ardae_hist2d_wide: .*1 <= nslots <= 65535"):
            hist(nslots=nslots)
    for kw in (dict(row_stride=0), dict(slot_stride=-1), dict(col_x=-1), dict(col_y=-1)):
        with pytest.raises(ValueError, match="^ardae_hist2d_wide: .*row_stride >= 1, slot_stride >= 0, col_x >= 0, col_y >= 0"):
            hist(**kw)
    for kw in (dict(pts=None), dict(counts=None)):
        with pytest.raises(ValueError, match="^ardae_hist2d_wide: .*must not be NULL"):
            hist(**kw)
    assert "stream" not in launches                                              # the stream was passed: none was fetched


def test_package_engine_and_header_expose_the_new_surface():
    assert net.GaussianDiagnostics is V.GaussianDiagnostics
    for m in ("latent_histograms", "data_histograms", "run", "final_pass"):
        assert callable(getattr(net.GaussianDiagnostics, m))
    assert callable(net.VaeEngine.diagnostics) and callable(net.PosteriorDiagnostics.final_pass)
    params = [p for p, _, _ in L.PROTOTYPES["ardae_hist2d_wide"][1]]
    assert params == ["pts", "n", "row_stride", "nslots", "slot_stride", "col_x", "col_y", "lo", "hi", "bins", "counts", "stream"]
    assert L.PROTOTYPES["ardae_hist2d_wide"] == L.PROTOTYPES["ardae_hist2d"] and L.EXPORTS["ardae_hist2d_wide"] == L.EXPORTS["ardae_hist2d"]
    assert hasattr(L.lib(), "ardae_hist2d_wide")                                # ... and the built library has the symbol
    assert L.CONSTANTS["ARDAE_ABI_VERSION"] == 1
    assert "eng.diagnostics(" in net.vae.__doc__
