"""Every device draw against the host reference oracle/philox_ref.py (which tests/test_philox.py pins to the Random123 known-answer
vectors): words, uniforms, Bernoullis and fused-vs-separate draws bit for bit, normals against float64 within NORMAL_TOL.

Keys are wide on purpose: 64-bit seeds, offsets with high bits (every host-side draw has bit 63 set), carries into the high offset
word that happen only through the step state, positions in a draw beyond 2^32 counters."""
import functools

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout, rng
from oracle import philox_ref as P
from score_gpu_checks import Harness, flat_of
from score_gpu_checks import init_params as dae_init_params
from score_restate import ARDAE
from test_fit_gpu import GenHarness
from test_fit_gpu import init_params as gen_init_params
from test_philox import EDGE_OFFSET, EDGE_SEED, EDGES

pytestmark = pytest.mark.gpu

# max |device normal - float64 reference|.  MEASURED_E is the worst element of the 2^20-element draw (seed 123, offset HOST_STREAM)
# on an MI355X: 6.8951e-07, at element 939155 (value +3.9457), mean error 4.3e-08.  The normals go through the hardware log2 / sin /
# cos units (csrc/philox.h), whose error cannot be derived from the instruction set's documentation; fp32 rounding of the result alone
# gives up to 5.77 * 2^-24 = 3.4e-7.  The error is not localised: every eighth of a revolution has a worst element of 4.7 - 6.9e-07,
# and it grows with the radius (1.7 - 2.6e-07 of it, three to four fp32 ulps).  The bound is 4 E = 2.76e-06: the worst element of
# another key may be worse than the worst of this one.  (The other keys of this file reach 5.0e-07 on their few thousand elements.)
MEASURED_E = 6.9e-7
NORMAL_TOL = 4 * MEASURED_E

HOST = rng.HOST_STREAM
WIDE_SEED = 0x9E3779B97F4A7C15
# (seed, offset, rng_offset of the step state or None)
KEYS = [(0, 0, None),
        (WIDE_SEED, 0xFFFFFFFF, None),
        (123, 1 << 32, None),
        (0x5EED, HOST | 7, None),
        (991, 0xFFFFFFFF, 1),                      # the carry into the high offset word happens only through the state
        (7, 2 ** 64 - 1, 16),                      # wraps modulo 2^64
        (0xFFFFFFFF00000000, 5, 1 << 40)]
KEY_IDS = ["zero", "wide_seed", "offset_2p32", "host_stream", "state_carry", "state_wrap", "high_seed_state_2p40"]
LENGTHS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 3074]
GUARD = 8


def make_state(rng_offset):
    """The 32-byte step state with rng_offset as its Philox base offset (None: no state)."""
    if rng_offset is None:
        return None
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    L.call("ardae_step_state_advance", state, rng_offset, 1e-3, 0.5, 0.999)
    return state


def normal_at(n, seed, offset, state=None, first=0, out=None):
    out = torch.empty(n, device="cuda") if out is None else out
    L.call("ardae_philox_normal_at", out, n, seed, offset, state, first)
    return out


def uniform(n, seed, offset, out=None):
    out = torch.empty(n, device="cuda") if out is None else out
    L.call("ardae_philox_uniform", out, n, seed, offset)
    return out


@functools.lru_cache(maxsize=None)
def ref_normal(seed, offset, first, n):
    z = P.normal(seed, offset, first, n)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def ref_uniform(seed, offset, n):
    u = P.uniform(seed, offset, n)
    u.setflags(write=False)
    return u


def max_err(got, want64):
    return float(np.max(np.abs(got.detach().cpu().numpy().astype(np.float64).reshape(-1) - want64.reshape(-1))))


def assert_normal(got, want64, what):
    assert bool(torch.isfinite(got).all()), what
    e = max_err(got, want64)
    print(f"{what}: max |device - float64| = {e:.3e} (bound {NORMAL_TOL:.1e})")
    assert e < NORMAL_TOL, (what, e)


def bits_equal(got, want32):
    return np.array_equal(got.detach().cpu().numpy().reshape(-1).view(np.uint32), np.ascontiguousarray(want32).reshape(-1).view(np.uint32))


# ---- the one measured tolerance ----------------------------------------------------------------------------------------------------
def test_normal_error_against_float64_is_within_the_recorded_bound():
    n = 1 << 20
    got = normal_at(n, 123, HOST)
    want = ref_normal(123, HOST, 0, n)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    worst = int(err.argmax())
    print(f"E = max |device - float64| over 2^20 normals (seed 123, offset HOST_STREAM) = {err.max():.4e} at element {worst} "
          f"(value {want[worst]:+.6f}); mean error {err.mean():.3e}; recorded E {MEASURED_E:.1e}, bound {NORMAL_TOL:.1e}")
    # where the error sits: by radius and by angle (revolutions) of the element's Box-Muller pair
    w = P.words(123, HOST, P.counters(0, n // 4)).reshape(-1, 2)
    rev = np.repeat(P.u01_open(w[:, 1]), 2)
    rad = np.repeat(np.sqrt(-2.0 * np.log(P.u01_open(w[:, 0]))), 2)
    for lo in np.arange(0.0, 1.0, 0.125):
        m = (rev > lo) & (rev <= lo + 0.125)
        print(f"  angle ({lo:.3f}, {lo + 0.125:.3f}] rev: max error {err[m].max():.3e}")
    for lo, hi in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 6)):
        m = (rad >= lo) & (rad < hi)
        print(f"  radius [{lo}, {hi}): max error {err[m].max():.3e}, relative to the radius {np.max(err[m] / np.maximum(rad[m], 1e-30)):.3e}")
    assert bool(torch.isfinite(got).all())
    assert err.max() < NORMAL_TOL


# ---- keys, lengths, tails, alignment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,offset,rng_offset", KEYS, ids=KEY_IDS)
def test_uniform_is_the_reference_bit_for_bit(seed, offset, rng_offset):
    """ardae_philox_uniform takes no state: the key's effective offset is passed by value."""
    off = P.step_offset(offset, rng_offset or 0)
    want = ref_uniform(seed, off, max(LENGTHS))
    for n in LENGTHS:
        buf = torch.full((n + GUARD,), float("nan"), device="cuda")
        uniform(n, seed, off, out=buf)
        assert bits_equal(buf[:n], want[:n]), n
        assert bool(torch.isnan(buf[n:]).all()), f"n={n}: wrote past the end"


@pytest.mark.parametrize("seed,offset,rng_offset", KEYS, ids=KEY_IDS)
def test_normal_at_is_the_reference_at_every_length_and_alignment(seed, offset, rng_offset):
    state = make_state(rng_offset)
    off = P.step_offset(offset, rng_offset or 0)
    want = ref_normal(seed, off, 0, max(LENGTHS))
    worst = 0.0
    for n in LENGTHS:
        aligned = None
        for shift in (0, 1, 2, 3):                  # views at element offsets 1 .. 3 of an aligned buffer: the kernel's scalar path
            buf = torch.full((shift + n + GUARD,), float("nan"), device="cuda")
            assert buf.data_ptr() % 16 == 0
            normal_at(n, seed, offset, state, 0, out=buf[shift:shift + n])
            assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + n:]).all()), f"n={n} shift={shift}: wrote outside [0, n)"
            got = buf[shift:shift + n].clone()
            if shift == 0:
                aligned = got
                assert bool(torch.isfinite(got).all())
                worst = max(worst, max_err(got, want[:n]))
                assert worst < NORMAL_TOL, (n, worst)
            else:
                assert torch.equal(got, aligned), f"n={n}: the view at element offset {shift} got other numbers"
    print(f"seed {seed:#x} offset {offset:#x} state {rng_offset}: max |device - float64| = {worst:.3e}")


def test_high_words_of_offset_and_seed_are_used():
    n = 64
    for seed, offset in ((123, 5), (WIDE_SEED, HOST | 1)):
        base_n, base_u = normal_at(n, seed, offset), uniform(n, seed, offset)
        for s2, o2 in ((seed, (offset + 2 ** 32) % 2 ** 64), ((seed + 2 ** 32) % 2 ** 64, offset), (seed, offset ^ HOST), (seed ^ (1 << 63), offset)):
            other_n, other_u = normal_at(n, s2, o2), uniform(n, s2, o2)
            assert not torch.equal(other_n, base_n) and not torch.equal(other_u, base_u), (hex(s2), hex(o2))
            assert bits_equal(other_u, ref_uniform(s2, o2, n))
            assert_normal(other_n, ref_normal(s2, o2, 0, n), f"seed {s2:#x} offset {o2:#x}")


# ---- position in the draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [4 * (2 ** 32 - 2), 1 << 63, 2 ** 64 - 64], ids=["counter_crosses_2p32", "element_2p63", "last_64_elements"])
@pytest.mark.parametrize("seed,offset,rng_offset", [KEYS[3], KEYS[4]], ids=[KEY_IDS[3], KEY_IDS[4]])
def test_normal_at_deep_into_a_draw(seed, offset, rng_offset, first):
    state = make_state(rng_offset)
    off = P.step_offset(offset, rng_offset or 0)
    for n in (16, 14):
        buf = torch.full((n + GUARD,), float("nan"), device="cuda")
        normal_at(n, seed, offset, state, first, out=buf)
        assert bool(torch.isnan(buf[n:]).all())
        assert_normal(buf[:n], ref_normal(seed, off, first, n), f"first_element {first:#x} n={n}")


def test_pieces_of_a_draw_are_the_draw():
    seed, offset, state = WIDE_SEED, (1 << 40) | 9, make_state(2 ** 32 - 1)
    whole = normal_at(4099, seed, offset, state)
    assert_normal(whole, ref_normal(seed, P.step_offset(offset, 2 ** 32 - 1), 0, 4099), "whole draw")
    for lo, hi in ((0, 1024), (1024, 2052), (2052, 4099)):
        assert torch.equal(normal_at(hi - lo, seed, offset, state, lo), whole[lo:hi]), (lo, hi)
    with pytest.raises(ValueError):
        normal_at(8, seed, offset, state, 2)


def test_the_other_normal_entry_points_are_normal_at():
    seed, offset, n = 0xFFFFFFFF00000000 | 77, HOST | (1 << 32) | 3, 1027
    plain = torch.empty(n, device="cuda")
    L.call("ardae_philox_normal", plain, n, seed, offset)
    assert torch.equal(plain, normal_at(n, seed, offset, None, 0))
    assert_normal(plain, ref_normal(seed, offset, 0, n), "ardae_philox_normal")
    state = make_state(0xFFFFFFFF)
    dev = torch.empty(n, device="cuda")
    L.call("ardae_philox_normal_dev", dev, n, seed, state, offset)
    assert torch.equal(dev, normal_at(n, seed, offset, state, 0))
    assert_normal(dev, ref_normal(seed, P.step_offset(offset, 0xFFFFFFFF), 0, n), "ardae_philox_normal_dev")
    assert not torch.equal(dev, plain)


# ---- the ends of the word-to-uniform maps -------------------------------------------------------------------------------------------
def test_edge_counters():
    """u = 1 (radius 0), u = 2^-24 (the largest radius), angle one revolution and 2^-24 of one; uniforms 0 and 1 - 2^-24."""
    for counter, word, top in EDGES:
        got = normal_at(4, EDGE_SEED, EDGE_OFFSET, None, 4 * counter)
        want = ref_normal(EDGE_SEED, EDGE_OFFSET, 4 * counter, 4)
        assert_normal(got, want, f"counter {counter} word {word} top bits {top:#08x}")
        g = got.cpu().numpy()
        if word in (0, 2) and top == 0xFFFFFF:
            assert g[word] == 0 and g[word + 1] == 0, (counter, g)               # exactly +-0, not a denormal and not NaN (sqrt(-0))
    # ardae_philox_uniform starts at counter 0: one draw that reaches the last edge counter, checked on the device
    n = 4 * (max(c for c, _, _ in EDGES) + 1)
    u = uniform(n, EDGE_SEED, EDGE_OFFSET)
    assert bool((u >= 0).all()) and bool((u < 1).all())
    for counter, word, top in EDGES:
        got = u[4 * counter:4 * counter + 4].cpu().numpy()
        assert np.array_equal(got, P.uniform(EDGE_SEED, EDGE_OFFSET, 4, first_element=4 * counter))
        assert got[word] == (0.0 if top == 0 else np.float32(1 - 2.0 ** -24))


# ---- Bernoulli ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 4), (3, 7), (257, 5), (5, 784)])
def test_bernoulli_is_the_reference_exactly(rows, cols):
    seed, offset = WIDE_SEED, HOST | (1 << 32) | 3
    u = ref_uniform(seed, offset, rows * cols)
    g = np.random.default_rng(rows * 1000 + cols)
    base = g.random(cols).astype(np.float32)
    base[0] = 0.0
    if cols > 1:
        base[1] = 1.0
    probe = sorted({0} if cols == 1 else {2, 3, cols - 1})         # columns of row 0 whose probability is set to the element's own uniform
    at, above = base.copy(), base.copy()
    for c in probe:
        at[c] = u[c]
        above[c] = np.nextafter(u[c], np.float32(1))
    cases = [base, at, above, np.zeros(cols, np.float32), np.ones(cols, np.float32)]
    outs = []
    for p in cases:
        buf = torch.full((rows * cols + GUARD,), float("nan"), device="cuda")
        L.call("ardae_bernoulli", torch.from_numpy(p).cuda(), rows, cols, buf, seed, offset)
        assert bool(torch.isnan(buf[rows * cols:]).all())
        got = buf[:rows * cols].cpu().numpy().reshape(rows, cols)
        assert np.array_equal(got, P.bernoulli(p, rows, cols, seed, offset))
        outs.append(got)
    for c in probe:
        assert outs[1][0, c] == 0.0, f"column {c}: u < p must be strict"
        assert outs[2][0, c] == 1.0, f"column {c}: p one ulp above u"
    assert (outs[0][:, 0] == 0).all() and (cols == 1 or (outs[0][:, 1] == 1).all())
    assert (outs[3] == 0).all() and (outs[4] == 1).all()


# ---- the host stream ----------------------------------------------------------------------------------------------------------------
def test_host_stream_draws_are_the_reference_at_consecutive_offsets():
    before = rng.get_state()
    try:
        s = 0xFFFFFFFF00000123
        net.manual_seed(s)
        z = net.rng.normal((10,), "cuda", first_element=8)
        assert rng.get_state()["offset"] == 1
        u = net.rng.uniform((7,), "cuda")
        assert rng.get_state()["offset"] == 2
        probs = torch.rand(3, 5, generator=torch.Generator().manual_seed(0)).cuda()
        x = net.data.dynamic_binarize(probs)
        assert rng.get_state() == {"seed": s, "offset": 3}
        assert_normal(z, ref_normal(s, HOST | 0, 8, 10), "rng.normal")
        assert bits_equal(u, P.uniform(s, HOST | 1, 7))
        assert np.array_equal(x.cpu().numpy(), P.bernoulli(probs.cpu().numpy().reshape(-1), 1, 15, s, HOST | 2).reshape(3, 5))
    finally:
        rng.manual_seed(before["seed"], before["offset"])


# ---- draws fused into their consumers, under wide keys --------------------------------------------------------------------------------
FUSED_RNG_OFFSET, FUSED_FIRST_ROW = 2 ** 32 - 1, 2 ** 33 + 8


def test_latent_perturb_draw_under_wide_keys():
    B, nz, z = 3, 128, 8
    assert L.query("ardae_latent_perturb_draw_ok", nz, 1, z) == 1
    g = torch.Generator().manual_seed(B + nz + z)
    z0 = torch.randn(B, z, generator=g).cuda()
    latent = (z0[:, None, :].cpu() + 0.05 * torch.randn(B, nz, z, generator=g)).cuda().contiguous()
    seed, k_xi, k_eps, first = WIDE_SEED, (1 << 40) | 4, (1 << 40) | 5, FUSED_FIRST_ROW
    state = make_state(FUSED_RNG_OFFSET)
    xi, eps = normal_at(B * nz, seed, k_xi, state, first), normal_at(B * nz * z, seed, k_eps, state, first * z)
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    xbar, sigma, std_b = new(B * nz, z), new(B * nz), new(B)
    L.call("ardae_latent_perturb", latent, z0, xi, eps, B, nz, z, 1e4, 0.1, xbar, sigma, std_b)
    xbar2, sigma2, std_b2, eps2 = new(B * nz, z), new(B * nz), new(B), new(B * nz, z)
    L.call("ardae_latent_perturb_draw", latent, z0, B, nz, z, 1e4, 0.1, seed, k_xi, k_eps, state, first, xbar2, sigma2, eps2, std_b2)
    torch.cuda.synchronize()
    assert torch.equal(eps2.reshape(-1), eps), "eps_out is not ardae_philox_normal_at's"
    assert torch.equal(std_b2, std_b) and torch.equal(sigma2, sigma) and torch.equal(xbar2, xbar)       # sigma = std_b * xi: xi bit for bit
    assert_normal(eps2, ref_normal(seed, P.step_offset(k_eps, FUSED_RNG_OFFSET), first * z, B * nz * z), "latent_perturb_draw eps")
    assert_normal(xi, ref_normal(seed, P.step_offset(k_xi, FUSED_RNG_OFFSET), first, B * nz), "latent_perturb_draw xi")


def test_dae_perturb_loss_grads_draws_under_wide_keys():
    B, ns, d, h, nl, kind, act = 5, 12, 3, 64, 2, "grad", "softplus"          # 60 rows: one partial 64-row tile
    spec = layout.dae_spec(kind, d, h, nl)
    hn = Harness(ARDAE, kind, d, h, nl, act, flat_of(dae_init_params(spec, 9), spec))
    assert L.query("ardae_dae_perturb_fused_ok", hn.d, ns) == 1
    N = B * ns
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(B)).cuda()
    delta, seed, k_sigma, k_eps, first = 0.7, WIDE_SEED, (1 << 40) | 3, (1 << 40) | 4, FUSED_FIRST_ROW
    state = make_state(FUSED_RNG_OFFSET)
    ws = torch.empty(L.query("ardae_cdae_workspace_floats", hn.d, N, 1, 1), device="cuda")
    loss, grads = torch.zeros(1, device="cuda"), torch.full_like(hn.params, float("nan"))
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    xbar, sigma, eps = new(N, d), new(N), new(N, d)
    L.call("ardae_dae_perturb_loss_grads", hn.d, hn.params, hn.packed, x, B, ns, delta, seed, k_sigma, k_eps, state, first, xbar, sigma, eps, ws,
           ws.numel(), loss, grads)
    torch.cuda.synchronize()
    n_ref, eps_ref = normal_at(N, seed, k_sigma, state, first), normal_at(N * d, seed, k_eps, state, first * d)
    assert torch.equal(eps.reshape(-1), eps_ref), "eps_out is not ardae_philox_normal_at's"
    assert torch.equal(sigma, delta * n_ref), "sigma is not delta * ardae_philox_normal_at's draw"
    xbar_ref = torch.empty(N, d, device="cuda")
    L.call("ardae_dae_perturb", x, sigma, eps, B, ns, d, xbar_ref)
    assert torch.equal(xbar, xbar_ref) and bool(torch.isfinite(loss).all())
    assert_normal(eps, ref_normal(seed, P.step_offset(k_eps, FUSED_RNG_OFFSET), first * d, N * d), "dae_perturb_loss_grads eps")
    assert_normal(n_ref, ref_normal(seed, P.step_offset(k_sigma, FUSED_RNG_OFFSET), first, N), "dae_perturb_loss_grads sigma / delta")


def test_gen_draw_forward_draws_under_wide_keys():
    B, zd, h, nl, act = 70, 2, 64, 2, "relu"                                     # two 64-row tiles, the second partial
    hn = GenHarness(zd, h, nl, act, gen_init_params(layout.gen_spec(2, h, zd, nl), 5))
    assert L.query("ardae_gen_draw_fused_ok", *hn.net) == 1
    seed, off = WIDE_SEED, (1 << 62) | (1 << 40) | 3
    state = make_state(FUSED_RNG_OFFSET)
    z_ref = normal_at(B * zd, seed, off, state, 0)
    z, ws, x = torch.full((B, zd), float("nan"), device="cuda"), hn.workspace(B), torch.empty(B, 2, device="cuda")
    L.call("ardae_gen_draw_forward", *hn.net, hn.params, hn.packed, B, seed, off, state, z, ws, ws.numel(), x)
    torch.cuda.synchronize()
    assert torch.equal(z.reshape(-1), z_ref), "z_out is not ardae_philox_normal_at's"
    assert bool(torch.isfinite(x).all())
    assert_normal(z, ref_normal(seed, P.step_offset(off, FUSED_RNG_OFFSET), 0, B * zd), "gen_draw_forward z")


# ---- the consumer of the uniforms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 0.5, 2.0 / 3.0])
def test_relaxed_bernoulli_at_the_ends_of_the_uniform(T):
    """sample = sigmoid((logit + log(u / (1 - u) + 1e-20)) / T) at the smallest and largest uniforms ardae_philox_uniform can give.
    2e-6: fp32 logf / expf and max |y sigmoid'(y)| = 0.22 (the bound of test_forward_and_generate_return_decoder_sample)."""
    us = np.array([0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24], dtype=np.float32)
    logits = np.array([-90, -20, -1e-3, 0, 3, 20, 90], dtype=np.float32)
    u, logit = (a.reshape(-1).copy() for a in np.meshgrid(us, logits, indexing="ij"))
    n = u.size
    sample, mean = torch.full((n + GUARD,), float("nan"), device="cuda"), torch.full((n + GUARD,), float("nan"), device="cuda")
    L.call("ardae_relaxed_bernoulli", torch.from_numpy(logit).cuda(), torch.from_numpy(u).cuda(), n, T, sample, mean)
    assert bool(torch.isnan(sample[n:]).all()) and bool(torch.isnan(mean[n:]).all())
    u64, l64, T64 = u.astype(np.float64), logit.astype(np.float64), np.float64(np.float32(T))
    sigmoid = lambda y: np.where(y >= 0, 1.0 / (1.0 + np.exp(-np.abs(y))), np.exp(-np.abs(y)) / (1.0 + np.exp(-np.abs(y))))
    want = sigmoid((l64 + np.log(u64 / (1.0 - u64) + 1e-20)) / T64)
    for name, got, ref in (("sample", sample[:n], want), ("mean", mean[:n], sigmoid(l64))):
        got = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), name
        e = np.abs(got - ref)
        print(f"T={T:.4f} {name}: max error {e.max():.2e} at u={u[e.argmax()]} logit={logit[e.argmax()]}")
        assert e.max() < 2e-6, (name, float(e.max()))
