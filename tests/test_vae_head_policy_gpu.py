"""What ardae_vae_head runs at variant 0 (the library's choice), per Gaussian-posterior kind: the family's fused form where
ardae_vae_head_fused_ok answers 1, the unfused launches where it answers 0, and the unfused launches everywhere under
ARDAE_VAE_HEAD_UNFUSED=1 (ARDAE_DEBUG_KNOBS=1).  Every comparison is bit for bit (the same launches must have run), on B = 9 rows - one past the
head's 8-row tile - with NaN-filled outputs, for the library's own draw and for an injected eps."""
import os
import subprocess
import sys

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 9
KEYS = ("mu", "lv", "z", "eps", "kld")
KNOB_ENV = {"ARDAE_DEBUG_KNOBS": "1", "ARDAE_VAE_HEAD_UNFUSED": "1"}
# name: (constructor, width of the hidden rows the head reads, what ardae_vae_head_fused_ok must answer - None: whatever the library says)
CASES = {
    "kind8_aligned": (lambda: net.MNISTVAE(input_dim=12, h_dim=40, z_dim=8, nonlinearity="softplus", num_hidden_layers=2), 40, 1),
    "kind8_unaligned": (lambda: net.MNISTVAE(input_dim=12, h_dim=42, z_dim=6, nonlinearity="softplus", num_hidden_layers=2), 42, None),
    "kind9": (lambda: net.ToyVAE(input_dim=2, h_dim=40, z_dim=2, nonlinearity="softplus", num_hidden_layers=1), 40, None),
    "kind11": (lambda: net.MNISTConvVAE(z_dim=6, nonlinearity="softplus"), 800, 1),
    "kind12": (lambda: net.MNISTResConvVAE(z_dim=6, c_dim=42), 42, 0),
}


def head(m, hid, variant, eps):
    out = {k: torch.full((B, m.z_dim), float("nan"), device=DEV) for k in KEYS[:4]}
    out["kld"] = torch.full((B,), float("nan"), device=DEV)
    L.call("ardae_vae_head", m._desc, m._flat, m._packed_weights(), hid, eps, B, 123, 5, None, variant, out["mu"], out["lv"], out["z"], out["eps"],
           out["kld"])
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    return out


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize("name", list(CASES))
def test_variant_0_is_the_documented_choice(name):
    ctor, h, want_ok = CASES[name]
    torch.manual_seed(len(name))
    m = ctor().to(DEV)
    unfused_knob = os.environ.get("ARDAE_DEBUG_KNOBS") == "1" and os.environ.get("ARDAE_VAE_HEAD_UNFUSED") == "1"
    ok = L.query("ardae_vae_head_fused_ok", m._desc)
    assert ok in (0, 1) and (want_ok is None or ok == want_ok)
    hid = torch.nn.functional.softplus(torch.randn(B, h)).to(DEV).contiguous()
    given = torch.randn(B, m.z_dim).to(DEV)
    for eps in (None, given):
        auto, fused, unfused = head(m, hid, 0, eps), head(m, hid, 1, eps), head(m, hid, 2, eps)
        picked = fused if ok and not unfused_knob else unfused
        print(f"{name} ({'own draw' if eps is None else 'injected eps'}): fused_ok {ok}, knob {int(unfused_knob)}, variants 1 and 2 "
              f"{'agree in every bit: the comparison does not discriminate' if same(fused, unfused) else 'differ: the comparison discriminates'}")
        assert same(auto, picked)


def test_variant_0_under_the_unfused_knob():
    """The library reads its debug knobs once per process, so the test above is re-run in a child process with the knob set: there variant 0 is
    the unfused launches for every case."""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "variant_0_is_the_documented_choice"], env=dict(os.environ, **KNOB_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"{len(CASES)} passed" in r.stdout and r.stdout.count("knob 1") == 2 * len(CASES), r.stdout[-1000:]
