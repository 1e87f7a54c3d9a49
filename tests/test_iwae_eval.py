"""The IWAE evaluator's host side (no GPU): chunk planning, and the refusals of the evaluator and of its two ABI entries, all of which
come before anything is launched."""
import types

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L

plan_chunks = net.plan_chunks


# ---- plan_chunks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,per_image,budget", [(1, 10, 40), (3, 10, 40), (4, 10, 40), (7, 10, 40), (8, 10, 79), (2048, 1000, 700_000),
                                                (10_000, 333, 10 ** 6), (10_001, 7, 10 ** 9), (37, 5, 20)])
def test_plan_chunks_covers_the_set_once_within_the_budget(N, per_image, budget):
    chunks = plan_chunks(N, 16, per_image, budget)
    assert chunks[0][0] == 0 and chunks[-1][1] == N
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))                # [0, N) exactly once, in order
    assert all(s % 4 == 0 and s < e for s, e in chunks)                        # a chunk starts on a Philox counter
    assert all((e - s) * per_image <= budget for s, e in chunks)
    assert all((e - s) % 4 == 0 for s, e in chunks[:-1])                       # only the last chunk is ragged
    assert len(chunks) == -(-N // max(e - s for s, e in chunks))               # ... and no chunk is needlessly short


def test_plan_chunks_cases_of_the_issue():
    assert plan_chunks(7, 16, 10, 40) == [(0, 4), (4, 7)]                      # N = 7 under a 4-image budget
    assert plan_chunks(7, 16, 10, 10 ** 6) == [(0, 7)]
    with pytest.raises(ValueError, match="a chunk of 4 images needs 40 floats"):
        plan_chunks(7, 16, 10, 39)                                             # below one chunk of 4 images
    with pytest.raises(ValueError, match="a chunk of 4 images needs 40 floats"):
        plan_chunks(2, 16, 10, 39)                                             # ... even where the set is smaller than that
    with pytest.raises(ValueError, match="rows"):
        plan_chunks(8, 2 ** 30, 1, 10 ** 6)                                    # 4 images are more rows than the ABI's int counts


def test_plan_chunks_takes_a_need_that_is_not_proportional():
    need = lambda c: 1000 + 10 * c                                             # noqa: E731  (a workspace query with a fixed part)
    chunks = plan_chunks(100, 16, need, 1000 + 10 * 24)
    assert chunks == [(0, 20), (20, 40), (40, 60), (60, 80), (80, 100)]        # 24 fit; five equal chunks of 20 cover the set
    assert all(need(e - s) <= 1240 for s, e in chunks)
    with pytest.raises(ValueError):
        plan_chunks(100, 16, need, 1039)
    # the row limit bounds a chunk too
    assert max(e - s for s, e in plan_chunks(64, 2 ** 27, 1, 10 ** 9)) * 2 ** 27 <= 2 ** 31 - 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _model(z_dim=8):
    return net.MNISTIPVAE(input_dim=24, noise_dim=10, h_dim=64, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=z_dim)


@pytest.fixture
def launches(monkeypatch):
    """Every launch goes through _lib._invoke and fetches the stream: record both."""
    seen = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: seen.append("stream") or types.SimpleNamespace(cuda_stream=0))
    invoke = L._invoke
    monkeypatch.setattr(L, "_invoke", lambda name, args: seen.append(name) or invoke(name, args))
    return seen


def test_evaluator_refuses_bad_inputs_before_any_launch(launches):
    with pytest.raises(NotImplementedError, match="z_dim 65 > 64"):
        net.IwaeEvaluator(_model(65), 256)
    with pytest.raises(AssertionError, match="sample_size >= 2 . z_dim"):       # ivae/mnist.py:382
        net.IwaeEvaluator(_model(8), 15)
    ev = net.IwaeEvaluator(_model(8), 16)
    x = torch.zeros(5, 24)
    with pytest.raises(TypeError, match="x_all: expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        ev.evaluate(x)
    with pytest.raises(TypeError, match="x_all: expected a float32 tensor on the GPU, got torch.float64"):
        ev.evaluate_rows(x.double())
    with pytest.raises(TypeError, match="x_all: expected a float32 tensor on the GPU"):
        ev.evaluate_rows(x.numpy())
    with pytest.raises(ValueError, match="x_all must be contiguous"):
        ev.evaluate_rows(torch.zeros(24, 5).t())
    assert launches == []


def test_evaluator_checks_injected_noise(launches):
    """The noise checks, on stand-ins for device tensors (is_cuda is all the checks read of the device)."""
    class OnDevice(torch.Tensor):
        is_cuda = True

    dev = lambda *shape: torch.zeros(*shape).as_subclass(OnDevice)             # noqa: E731
    ev = net.IwaeEvaluator(_model(8), 16)
    N = 5
    ok = ev._check_noise(N, dev(N, 16, 10), dev(N, 16, 8))
    assert ok[0].shape == (N, 16, 10) and ok[1].shape == (N, 16, 8)
    assert ev._check_noise(N, None, None) == (None, None)
    with pytest.raises(TypeError, match="enc_noise: expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        ev._check_noise(N, torch.zeros(N, 16, 10), None)
    with pytest.raises(TypeError, match="prop_noise: expected a float32 tensor on the GPU, got torch.float16"):
        ev._check_noise(N, None, dev(N, 16, 8).half())
    with pytest.raises(ValueError, match="prop_noise must be contiguous"):
        ev._check_noise(N, None, dev(N, 8, 16).transpose(1, 2))
    with pytest.raises(ValueError, match=r"enc_noise must be \[5, 16, 10\]"):
        ev._check_noise(N, dev(N, 16, 12), None)
    with pytest.raises(ValueError, match=r"prop_noise must be \[5, 16, 8\]"):
        ev._check_noise(N, None, dev(N + 1, 16, 8))
    with pytest.raises(ValueError, match="is one tensor"):
        ev._check_noise(N, (dev(N, 16, 10), dev(N, 16, 8)), None)
    aux = net.IwaeEvaluator(net.MNISTAuxIPVAE(input_dim=24, noise_dim=10, h_dim=48, z_dim=8), 16)
    with pytest.raises(ValueError, match="is the pair"):
        aux._check_noise(N, dev(N, 16, 18), None)
    toy = net.IwaeEvaluator(net.ToyAuxIPVAE(), 8)
    assert toy.ke == 64 and toy.noise_blocks == (8 * 2, 64 * 2) and toy.jitter == aux.jitter == 1e-5 and ev.jitter == 0.0
    with pytest.raises(ValueError, match=r"enc_noise\[1\] must be \[5, 64, 2\]"):
        toy._check_noise(N, (dev(N, 8, 2), dev(N, 8, 2)), None)
    assert launches == []


def test_abi_entries_check_their_arguments_before_any_hip_call(launches):
    f32 = torch.zeros(2, 4, 2)
    good = dict(B=2, ke=4, k=4, z=2, jitter=0.0, seed=1, offset=2, first=0)

    def proposal(zs=None, prop=None, out=None, **kw):
        a = dict(good, **kw)
        L.call("ardae_iwae_proposal", zs, prop, a["B"], a["ke"], a["k"], a["z"], a["jitter"], a["seed"], a["offset"], a["first"], out, out, None, None,
               None, None)

    # the converter: a CPU tensor, the wrong dtype
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        proposal(zs=f32)
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float64 on cpu"):
        proposal(prop=f32.double())
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):
        L.call("ardae_iwae_reduce", f32, None, None, 2, 4, None, None)
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.int64"):
        L.call("ardae_iwae_reduce", None, None, None, 2, 4, torch.zeros(2, dtype=torch.int64), None)
    assert launches == ["ardae_iwae_proposal"] * 2 + ["ardae_iwae_reduce"] * 2          # refused in the converter, nothing fetched or entered
    # the library's own validation, which runs before any HIP call
    for first in (1, 2, 3, 4 * 4 * 2 + 2):
        with pytest.raises(ValueError, match="^ardae_iwae_proposal: .*first_element must be a multiple of 4"):
            proposal(first=first)
    with pytest.raises(ValueError, match=r"^ardae_iwae_proposal: .*1 <= z <= 64 \(got z=65\)"):
        proposal(z=65, k=130, ke=130)
    with pytest.raises(ValueError, match="^ardae_iwae_proposal: .*1 <= z <= 64"):
        proposal(z=0)
    with pytest.raises(ValueError, match="^ardae_iwae_proposal: .*ke >= 2"):
        proposal(ke=1)
    with pytest.raises(ValueError, match="^ardae_iwae_proposal: .*B > 0"):
        proposal(B=0)
    with pytest.raises(ValueError, match="^ardae_iwae_proposal: .*jitter"):
        proposal(jitter=-1e-5)
    with pytest.raises(ValueError, match="^ardae_iwae_proposal: .*must not be NULL"):
        proposal()
    with pytest.raises(ValueError, match="^ardae_iwae_reduce: .*k >= 1"):
        L.call("ardae_iwae_reduce", None, None, None, 2, 0, None, None)
    with pytest.raises(ValueError, match="^ardae_iwae_reduce: .*NULL"):
        L.call("ardae_iwae_reduce", None, None, None, 2, 4, None, None)
    assert "stream" not in launches                                              # the stream was passed: none was fetched


def test_engine_and_package_expose_the_evaluator():
    assert callable(net.IwaeEvaluator) and callable(net.plan_chunks) and hasattr(net.ArdaeEngine, "evaluate_iws")
    assert L.EXPORTS["ardae_iwae_reduce"][0] is L.EXPORTS["ardae_iwae_proposal"][0]
    assert len(L.EXPORTS["ardae_iwae_proposal"][1]) == 16 and len(L.EXPORTS["ardae_iwae_reduce"][1]) == 7
    assert L.CONSTANTS["ARDAE_ABI_VERSION"] == 1
