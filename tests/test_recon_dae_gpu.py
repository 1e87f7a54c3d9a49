"""The reconstruction DAEs of models/dae/mlp.py on the device: net.MLPDAE / net.MLPCDAE, ardae_cdae_desc.kind 13, the entry points of
csrc/recon_dae.hip and the two score engines with them.

Bars: loss 2e-5 relative, x_bar, x_recon and every gradient tensor 1e-4 relative L2 against the reference's fp32 fixtures (tests/score_restate.py);
glogprob max(1e-4, 3 x the fixture's own fp32-to-float64 distance): the division by std^2 amplifies the cancellation in recon - x.  The float64
oracle is the restatement in tests/recon_restate.py, which tests/test_recon_dae.py pins to the reference's fp64 fixtures to 1e-12."""
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import philox_ref as P
from recon_restate import COND_IDS, UNCOND, add_noise, case, forward, glog_tol
from score_gpu_checks import STRIDE, Harness, dae_block, flat_of, guarded, init_params, sigma32
from score_restate import LOSS_TOL, TENSOR_TOL, load, rel, state_dict_of
from test_philox import EDGE_OFFSET, EDGE_SEED, EDGES

pytestmark = pytest.mark.gpu
NORMAL_TOL = 4 * 6.9e-7       # tests/test_philox_gpu.py: four times the measured worst distance of a device normal from float64 Box-Muller
NOISE = {"gaussian": 0, "uniform": 1}


class Kind:
    """What score_gpu_checks.Harness reads of a Family, for one network kind"""

    def __init__(self, kind_id, spec):
        self.kind_id, self._spec = {"res": kind_id}, spec

    def spec_of(self, kind, d, h, nl, c=0):
        return self._spec(d, c, h, nl)


K7 = Kind(7, lambda d, c, h, nl: layout.dae_plain_spec("res", d, h, nl))
K11 = Kind(11, lambda d, c, h, nl: layout.cdae_plain_spec("res", d, c, h, nl))
K13 = Kind(13, lambda d, c, h, nl: layout.recon_cdae_spec(d, c, h, nl, False))


def kind_of(conditional, enc_input):
    return K7 if not conditional else K11 if enc_input else K13


def fixture(golden_dir, fid):
    return load(os.path.join(golden_dir, f"recon_{'dae' if fid.startswith('n') else 'cdae'}_{fid}.npz"))


def module_of(fx):
    conditional, act, noise, enc_input, _, (d, c, h, nl), *_ = case(fx)
    kw = dict(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act, noise_type=noise)
    m = net.MLPCDAE(context_dim=c, enc_input=enc_input, **kw) if conditional else net.MLPDAE(**kw)
    m.load_state_dict(state_dict_of(fx))
    return m.cuda()


def context_rows(fx, ctx, B, S):
    """-> ((B, S) of the ABI call, ctx rows): one context per sample row, or - the fixture repeats it over S - one per image"""
    if ctx is None:
        return (B * S, 1), None
    if int(fx["rows"]):
        return (B * S, 1), ctx
    return (B, S), ctx.view(B, S, -1)[:, 0, :].contiguous()


def perturb(x, draw, B, ns, noise, sigma, block=None):
    """ardae_recon_perturb into guarded buffers -> xbar, ones, target"""
    N, d = B * ns, x.size(1)
    (xb_all, xbar), (sg_all, ones), (tg_all, target) = guarded(N, d), guarded(N), guarded(N, d)
    L.call("ardae_recon_perturb", x, draw, B, ns, d, noise, sigma, block, xbar, ones, target)
    for full in (xb_all, sg_all, tg_all):
        assert torch.isnan(full[N:]).all() and not torch.isnan(full[:N]).any()
    return xbar, ones, target


def assert_grads(grads, fx, what):
    for n, g in grads.items():
        assert not torch.isnan(g).any(), (what, n)
        e = rel(g, fx["g/" + n])
        assert e <= TENSOR_TOL, f"{what}: {n} relL2 {e:.2e}"


# ---- 1. the C ABI against every fixture of the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("fid", list(UNCOND) + COND_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    fx = fixture(golden_dir, fid)
    conditional, act, noise, enc_input, (B, S), (d, c, h, nl), p, x, ctx, std, draw = case(fx)
    N, k = B * S, kind_of(conditional, enc_input)
    hn = Harness(k, "res", d, h, nl, act, flat_of(p, k.spec_of("res", d, h, nl, c)), c)
    x, draw = x.cuda(), draw.cuda()
    if torch.is_tensor(std):        # a noise level per row: the reference's expressions row by row (the entry point takes one level)
        xbar, ones, target = add_noise(noise, x, std.cuda(), draw), torch.ones(N, device="cuda"), -x
    else:
        xbar, ones, target = perturb(x, draw, N, 1, NOISE[noise], std)
        assert torch.equal(ones, torch.ones(N, device="cuda")) and torch.equal(target, -x)
    e = rel(xbar.cpu(), fx["xbar"])
    print(f"{fid}: x_bar relL2 {e:.2e}")
    assert e <= TENSOR_TOL
    (Bc, Sc), crow = context_rows(fx, ctx, B, S)
    loss, grads, recon = hn.loss_grads(xbar, ones, target, crow, Bc, Sc)
    print(f"{fid}: loss {float(loss):.7f} (reference {float(fx['loss']):.7f}), x_recon relL2 {rel(recon, fx['x_recon']):.2e}")
    assert abs(float(loss) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    assert rel(recon, fx["x_recon"]) <= TENSOR_TOL
    assert_grads(grads, fx, fid)
    # the score: the network's output at x whatever sigma is passed, then the residual over std^2
    out = hn.score(x, None, crow, Bc, Sc)
    assert torch.equal(out, hn.score(x, torch.full((N,), float("nan")), crow, Bc, Sc))
    if torch.is_tensor(std):
        glog = (out - x.cpu()) / std ** 2
    else:
        buf = out.cuda()
        L.call("ardae_recon_score", buf, x, N, d, std, None, buf)            # out may alias recon
        glog = buf.cpu()
        assert rel(glog, (out - x.cpu()) / float(np.float32(std) * np.float32(std))) <= 1e-6
    bar = glog_tol(fx, TENSOR_TOL)
    e = rel(glog.reshape(-1), fx["glog"].reshape(-1))
    print(f"{fid}: glogprob relL2 {e:.2e} (bar {bar:.2e})")
    assert e <= bar
    if conditional and not int(fx["rows"]):        # one context per image, run as one per row: the same function
        loss2, grads2, recon2 = hn.loss_grads(xbar, ones, target, ctx, N, 1)
        assert abs(float(loss2) - float(loss)) <= LOSS_TOL * abs(float(loss)) and rel(recon2, recon) <= TENSOR_TOL
        assert_grads(grads2, fx, fid + " per row")


# ---- 2. the loss layer is reused: the modules against ardae_cdae_loss_grads on (x_bar, ones, -x), bit for bit; the module route ------
@pytest.mark.parametrize("fid", list(UNCOND) + COND_IDS)
def test_module_is_the_res_kind_loss_layer_on_ones_and_minus_x(golden_dir, fid):
    """MLPDAE: kind 7; MLPCDAE with enc_input=True: kind 11; enc_input=False: kind 13.  And the drop-in surface on the fixture: loss.backward()
    gives the reference's .grad, x_recon comes back detached, glogprob has the reference's shape."""
    fx = fixture(golden_dir, fid)
    conditional, act, noise, enc_input, (B, S), (d, c, h, nl), p, x, ctx, std, draw = case(fx)
    N, k = B * S, kind_of(conditional, enc_input)
    m = module_of(fx)
    assert m._desc.kind == k.kind_id["res"] and all(torch.equal(v.cpu(), p[n]) for n, v in m.state_dict().items())
    std_d = std.cuda() if torch.is_tensor(std) else std
    args = (torch.tensor(fx["x"]).cuda(),) + ((torch.tensor(fx["ctx"]).cuda(),) if conditional else ())
    recon, loss = m(*args, std_d, eps=draw.cuda())
    assert recon.shape == (N, d) and not recon.requires_grad and loss.dim() == 0 and loss.requires_grad
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"])) and rel(recon.cpu(), fx["x_recon"]) <= TENSOR_TOL
    xbar = m.add_noise(x.cuda(), std_d, eps=draw.cuda())
    hn = Harness(k, "res", d, h, nl, act, m.flat_params().detach().cpu(), c)
    abi_loss, abi_grads, abi_recon = hn.loss_grads(xbar, torch.ones(N), -x, ctx, N, 1)          # the module route: one context per row
    assert float(loss.detach()) == float(abi_loss) and torch.equal(recon.cpu(), abi_recon)
    for n, q in m.named_parameters():
        assert torch.equal(q.grad.cpu(), abi_grads[n]), n
        assert rel(q.grad.cpu(), fx["g/" + n]) <= TENSOR_TOL, n
    glog = m.glogprob(*args, std_d)
    assert glog.shape == ((B, S, d) if conditional else (N, d))
    assert rel(glog.cpu().reshape(-1), fx["glog"].reshape(-1)) <= glog_tol(fx, TENSOR_TOL)
    # std=None is self.std; eps=None is the module's own Philox draw, a fresh one per call
    m.std = 0.37
    call = lambda *a, **kw: float(m(*args, *a, **kw)[1].detach())
    assert call(eps=draw.cuda()) == call(0.37, eps=draw.cuda()) == call(torch.full((N, 1), 0.37, device="cuda"), eps=draw.cuda()) != float(loss.detach())
    a, b = call(), call()
    assert np.isfinite(a) and np.isfinite(b) and a != b
    assert torch.equal(m.glogprob(*args), m.glogprob(*args, 0.37))


@pytest.mark.parametrize("enc_input", [False, True])
@pytest.mark.parametrize("noise", ["gaussian", "uniform"])
def test_expanded_context_equals_repeated_rows(enc_input, noise):
    """A [B, 1, c] context expanded along dim 1 runs as (B, S); the same rows materialised run as (N, 1): the same loss and gradients."""
    B, S, d, c, h, nl = 6, 20, 3, 5, 64, 2
    g = torch.Generator().manual_seed(3)
    m = net.MLPCDAE(input_dim=d, context_dim=c, h_dim=h, num_hidden_layers=nl, nonlinearity="softplus", noise_type=noise, enc_input=enc_input)
    m.load_state_dict(init_params(layout.recon_cdae_spec(d, c, h, nl, enc_input), 8))
    m = m.cuda()
    x, ctx1 = torch.randn(B, S, d, generator=g).cuda(), torch.randn(B, 1, c, generator=g).cuda()
    draw = (torch.rand(B * S, d, generator=g) if noise == "uniform" else torch.randn(B * S, d, generator=g)).cuda()
    out = []
    for ctx in (ctx1.expand(B, S, c), ctx1.expand(B, S, c).contiguous()):
        m.zero_grad()
        recon, loss = m(x, ctx, 0.4, eps=draw)
        loss.backward()
        out.append((loss.detach().cpu(), recon.cpu(), [q.grad.cpu().clone() for q in m.parameters()], m.glogprob(x, ctx, 0.4).cpu()))
    (l0, r0, g0, s0), (l1, r1, g1, s1) = out
    assert abs(float(l0) - float(l1)) <= TENSOR_TOL * abs(float(l1)) and rel(r0, r1) <= TENSOR_TOL and rel(s0, s1) <= TENSOR_TOL
    assert all(rel(a, b) <= TENSOR_TOL for a, b in zip(g0, g1))
    with pytest.raises(ValueError, match="one row per sample row"):
        m(x, ctx1)


# ---- 3. kind 13: no sibling with equal bits - against kind 11 where the input half is silent, and against float64 ---------------------
SHAPES13 = [(4, 16, 2, 3, 64, 3, "softplus"), (5, 12, 3, 5, 100, 2, "elu"), (8, 8, 2, 2, 64, 1, "relu"), (16, 40, 8, 12, 128, 3, "softplus"),
            (7, 33, 5, 3, 96, 2, "tanh")]


@pytest.mark.parametrize("B,S,d,c,h,nl,act", SHAPES13, ids=[f"b{s[0]}_s{s[1]}_d{s[2]}_h{s[4]}_{s[6]}" for s in SHAPES13])
def test_kind_13_against_kind_11_with_a_silent_input_half_and_against_float64(B, S, d, c, h, nl, act):
    N = B * S
    g = torch.Generator().manual_seed(N + d)
    x, draw, ctx = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g), torch.randn(B, c, generator=g)
    xbar = x + 0.5 * draw
    spec13, spec11 = K13.spec_of("res", d, h, nl, c), K11.spec_of("res", d, h, nl, c)
    p = init_params(spec13, 4)
    # (a) against float64, the input half at work
    x64, _, loss64, g64 = forward({n: v.double() for n, v in p.items()}, act, "gaussian", x.double(), 0.5, draw.double(), ctx.double().repeat_interleave(S, 0))
    loss, grads, recon = Harness(K13, "res", d, h, nl, act, flat_of(p, spec13), c).loss_grads(xbar, torch.ones(N), -x, ctx, B, S)
    assert abs(float(loss) - float(loss64)) <= LOSS_TOL * abs(float(loss64))
    for n in grads:
        e = rel(grads[n], g64[n])
        print(f"kind 13 B={B} S={S} d={d} h={h} L={nl} {act} {n}: to float64 {e:.2e}")
        assert e <= TENSOR_TOL, (n, e)
    # (b) W1x = 0 against a kind-11 network whose W1a is zero: what reaches ctx_encode.* and W1c is the same
    first = "dae.layers.0.weight"
    p0 = dict(p)
    p0[first] = torch.cat([torch.zeros(h, d), p[first][:, d:]], 1)
    q = init_params(spec11, 6)
    q.update({n: v for n, v in p0.items() if n != first})
    q[first] = torch.cat([torch.zeros(h, h), p[first][:, d:]], 1)
    l13, g13, r13 = Harness(K13, "res", d, h, nl, act, flat_of(p0, spec13), c).loss_grads(xbar, torch.ones(N), -x, ctx, B, S)
    l11, g11, r11 = Harness(K11, "res", d, h, nl, act, flat_of(q, spec11), c).loss_grads(xbar, torch.ones(N), -x, ctx, B, S)
    assert abs(float(l13) - float(l11)) <= LOSS_TOL * abs(float(l11)) and rel(r13, r11) <= TENSOR_TOL
    for n in g13:
        a, b = (g13[n][:, d:], g11[n][:, h:]) if n == first else (g13[n], g11[n])
        assert rel(a, b) <= TENSOR_TOL, (n, rel(a, b))


# ---- 4. ardae_philox_uniform_at --------------------------------------------------------------------------------------------------------
def uniform_at(n, seed, offset, state, first):
    full, out = guarded(n)
    L.call("ardae_philox_uniform_at", out, n, seed, offset, state, first)
    torch.cuda.synchronize()
    assert torch.isnan(full[n:]).all()
    return out.cpu().numpy()


@pytest.mark.parametrize("with_state", [False, True])
def test_philox_uniform_at_is_the_host_reference_bit_for_bit(with_state):
    seed, offset = 0xC0FFEE, 5
    state = dae_block(3, 1.0, 0.1, 4) if with_state else None               # base offset 3 * STRIDE
    eff = P.step_offset(offset, 3 * STRIDE) if with_state else offset
    whole = P.uniform(seed, eff, 1024)
    for first in (0, 4, 64, 1, 2, 3, 5, 63, 130):
        for n in (1, 3, 4, 5, 63, 64, 257):
            got = uniform_at(n, seed, offset, state, first)
            assert got.tobytes() == whole[first:first + n].tobytes(), (first, n)
    assert uniform_at(64, seed, offset, state, 0).tobytes() != P.uniform(seed, eff + 1, 64).tobytes()
    # pieces of a draw are the draw
    cuts = [0, 1, 4, 9, 64, 67, 300, 557, 1024]
    pieces = np.concatenate([uniform_at(b - a, seed, offset, state, a) for a, b in zip(cuts, cuts[1:])])
    assert pieces.tobytes() == whole.tobytes()
    if not with_state:                  # the stand-alone draw from counter 0 is the same map
        u = torch.empty(1024, device="cuda")
        L.call("ardae_philox_uniform", u, 1024, seed, offset)
        assert u.cpu().numpy().tobytes() == whole.tobytes()


# ---- 5. the draw + perturb forms against the stand-alone draw followed by the unfused perturbation ------------------------------------
def draw_then_perturb(latent, src, z0, B, nz, ns, d, scale, noise, sigma, block, seed, first_row):
    N = B * nz * ns
    (dr_all, draw), (xb_all, xbar), (sg_all, ones), (tg_all, target) = guarded(N, d), guarded(N, d), guarded(N), guarded(N, d)
    L.call("ardae_philox_uniform_at" if noise else "ardae_philox_normal_at", draw, N * d, seed, 2, block, first_row * d)
    if latent:
        L.call("ardae_latent_recon_perturb", src, z0, draw, B, nz, ns, d, scale, noise, sigma, block, xbar, ones, target)
    else:
        L.call("ardae_recon_perturb", src, draw, B, ns, d, noise, sigma, block, xbar, ones, target)
    return (xbar, ones, target, draw), (xb_all, sg_all, tg_all, dr_all)


def draw_form(latent, src, z0, B, nz, ns, d, scale, noise, sigma, block, seed, first_row, offset=2):
    N = B * nz * ns
    (dr_all, draw), (xb_all, xbar), (sg_all, ones), (tg_all, target) = guarded(N, d), guarded(N, d), guarded(N), guarded(N, d)
    if latent:
        L.call("ardae_latent_recon_perturb_draw", src, z0, B, nz, ns, d, scale, noise, sigma, block, seed, offset, first_row, xbar, ones, target, draw)
    else:
        L.call("ardae_recon_perturb_draw", src, B, ns, d, noise, sigma, block, seed, offset, first_row, xbar, ones, target, draw)
    return (xbar, ones, target, draw), (xb_all, sg_all, tg_all, dr_all)


@pytest.mark.parametrize("latent", [False, True], ids=["broadcast", "latent"])
@pytest.mark.parametrize("noise", [0, 1], ids=["gaussian", "uniform"])
@pytest.mark.parametrize("d", [2, 3, 8])
def test_draw_forms_equal_the_two_launches_bit_for_bit(latent, noise, d):
    seed, scale = 99, 1.5
    block = dae_block(3, 1.0, 0.1, 4)
    s_block = sigma32(net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4), 2)
    for B, nz, ns in ((15, 1, 4), (16, 1, 4), (13, 1, 10)) if not latent else ((5, 6, 2), (4, 16, 1), (5, 13, 2)):      # N = 60, 64, 130
        N = B * nz * ns
        assert N in (60, 64, 130)
        g = torch.Generator().manual_seed(N + d)
        src, z0 = torch.randn(B * nz, d, generator=g).cuda(), (torch.randn(B, d, generator=g).cuda() if latent else None)
        for first_row in (0, 8):
            for sigma, blk in ((0.3, None), (123.0, block)):                 # with a block the argument is not read
                ref, ref_full = draw_then_perturb(latent, src, z0, B, nz, ns, d, scale, noise, sigma, blk, seed, first_row)
                got, got_full = draw_form(latent, src, z0, B, nz, ns, d, scale, noise, sigma, blk, seed, first_row)
                torch.cuda.synchronize()
                for name, a, b in zip(("xbar", "sigma_out", "target_out", "draw_out"), got, ref):
                    assert torch.equal(a, b), (name, N, d, first_row, blk is not None)
                for full in got_full + ref_full:
                    assert torch.isnan(full[N:]).all() and not torch.isnan(full[:N]).any()
                # and what they hold: the host's formula in the stated operation order
                xbar, ones, target, draw = (t.cpu() for t in got)
                s = float(np.float32(s_block if blk is not None else sigma))
                rows = src.cpu().repeat_interleave(ns, 0)
                if latent:
                    rows = (scale * (src.cpu().view(B, nz, d) - z0.cpu()[:, None, :])).view(B * nz, d).repeat_interleave(ns, 0)      # 1.5: exact in fp32
                assert torch.equal(ones, torch.ones(N)) and torch.equal(target, -rows)
                if noise:
                    assert 0.0 <= float(draw.min()) and float(draw.max()) < 1.0
                    assert torch.equal(xbar, rows + (float(np.float32(2.0) * np.float32(s)) * draw - s))      # each operation rounded in fp32
                else:
                    assert torch.equal(xbar, (rows.double() + s * draw.double()).float())         # one fma: a single rounding
                off = P.step_offset(2, 3 * STRIDE) if blk is not None else 2
                if noise:
                    assert draw.numpy().tobytes() == P.uniform(seed, off, N * d, first_element=first_row * d).tobytes()
                else:           # normals: the host's float64 Box-Muller on the same words, within tests/test_philox_gpu.py's bound
                    assert np.abs(draw.numpy().reshape(-1).astype(np.float64) - P.normal(seed, off, first_row * d, N * d)).max() < NORMAL_TOL


@pytest.mark.parametrize("noise", [0, 1], ids=["gaussian", "uniform"])
def test_unaligned_pointers_give_the_bits_of_the_16_byte_paths(noise):
    """d = 8: a counter's four elements lie in one row and every access is 16 bytes wide where the pointers allow; the same calls on views that start
    one float into their allocations take the element-by-element paths and must give the same bits."""
    B, nz, ns, d, seed = 5, 13, 2, 8, 31
    N = B * nz * ns
    g = torch.Generator().manual_seed(N)
    off1 = lambda t: torch.cat([torch.zeros(1), t.reshape(-1)]).cuda()[1:].view(t.shape)          # the same values, 4 bytes off a 16-byte boundary
    lat, z0, draw = torch.randn(B * nz, d, generator=g), torch.randn(B, d, generator=g), torch.rand(N, d, generator=g)
    out = lambda shift: torch.full((N * d + 1,), float("nan"), device="cuda")[int(shift):int(shift) + N * d].view(N, d)
    for latent in (False, True):
        outs = []
        for shift in (False, True):
            src, zz, dr = ((off1(t) if shift else t.cuda()) for t in (lat, z0, draw))
            xbar, target, fx, ft, fd = (out(shift) for _ in range(5))
            assert all((t.data_ptr() % 16 != 0) == shift for t in (src, zz, dr, xbar, target, fx, ft, fd))
            ones, fones = (torch.full((N,), float("nan"), device="cuda") for _ in range(2))
            if latent:
                L.call("ardae_latent_recon_perturb", src, zz, dr, B, nz, ns, d, 1.5, noise, 0.3, None, xbar, ones, target)
                L.call("ardae_latent_recon_perturb_draw", src, zz, B, nz, ns, d, 1.5, noise, 0.3, None, seed, 2, 8, fx, fones, ft, fd)
            else:
                L.call("ardae_recon_perturb", src, dr, B * nz, ns, d, noise, 0.3, None, xbar, ones, target)
                L.call("ardae_recon_perturb_draw", src, B * nz, ns, d, noise, 0.3, None, seed, 2, 8, fx, fones, ft, fd)
            score = out(shift)
            score.copy_(xbar)
            L.call("ardae_recon_score", score, target, N, d, 0.3, None, score)                  # in place
            torch.cuda.synchronize()
            assert torch.equal(ones, torch.ones(N, device="cuda")) and torch.equal(fones, ones)
            outs.append([t.clone() for t in (xbar, target, score, fx, ft, fd)])
        assert all(torch.equal(a, b) and not torch.isnan(a).any() for a, b in zip(*outs)), latent


def test_uniform_end_points():
    """u = 0 and u = 1 - 2^-24 (the counters tests/test_philox.py pins): x_bar is the host's formula in the stated operation order, bit for bit,
    from the draw form and from the unfused perturbation."""
    assert {t for _, _, t in EDGES} == {0x000000, 0xFFFFFF}
    x = torch.linspace(-1.7, 2.3, 4).view(4, 1).cuda()
    xh = x.cpu().numpy().reshape(-1)
    for counter, word, top in EDGES:
        u_want = np.float32(top) * np.float32(2.0 ** -24)
        assert u_want in (np.float32(0.0), np.float32(1.0 - 2.0 ** -24))
        want_draw = P.uniform(EDGE_SEED, EDGE_OFFSET, 4, first_element=4 * counter)
        assert want_draw[word] == u_want
        for s in (0.3, 1.25, 0.05):
            # d = 1: row r of the call is element 4 counter + r of the draw
            (xbar, ones, target, draw), _ = draw_form(False, x, None, 4, 1, 1, 1, 1.0, 1, s, None, EDGE_SEED, 4 * counter, offset=EDGE_OFFSET)
            dr = draw.cpu().numpy().reshape(-1)
            assert dr.tobytes() == want_draw.tobytes() == uniform_at(4, EDGE_SEED, EDGE_OFFSET, None, 4 * counter).tobytes()
            s32 = np.float32(s)
            want = (xh + ((np.float32(2.0) * s32) * dr - s32)).astype(np.float32)
            assert want.dtype == np.float32 and xbar.cpu().numpy().reshape(-1).tobytes() == want.tobytes()
            assert torch.equal(perturb(x, draw, 4, 1, 1, s)[0], xbar)
            xb = xbar.cpu().numpy().reshape(-1)
            assert xh[word] - s32 <= xb[word] <= xh[word] + s32 and (top != 0 or xb[word] == xh[word] - s32)


# ---- 6. engines ------------------------------------------------------------------------------------------------------------------------
def fresh(conditional, noise, enc_input=False, seed=21, d=2, c=3, h=64, nl=3, act="softplus"):
    kw = dict(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act, noise_type=noise)
    if conditional:
        m = net.MLPCDAE(context_dim=c, enc_input=enc_input, **kw)
        m.load_state_dict(init_params(layout.recon_cdae_spec(d, c, h, nl, enc_input), seed))
    else:
        m = net.MLPDAE(**kw)
        m.load_state_dict(init_params(layout.dae_plain_spec("res", d, h, nl), seed))
    return m.cuda()


def batches(conditional, n, B, S, d=2, c=3):
    out = []
    for s in range(n):
        g = torch.Generator().manual_seed(s)
        if conditional:
            mean = torch.randn(B, d, generator=g)
            out.append(((mean[:, None, :] + 0.5 * torch.randn(B, S, d, generator=g)).cuda(), torch.randn(B, c, generator=g).cuda(), mean.cuda()))
        else:
            out.append((torch.randn(B, d, generator=g).cuda(),))
    return out


def engine(conditional, m, cfg, B, S, **kw):
    return net.ArdaeCondScoreEngine(m, cfg, B, S, std_scale=1.5, **kw) if conditional else net.ArdaeScoreEngine(m, cfg, B, **kw)


ENGINE_CASES = [(False, "gaussian", False, False), (False, "uniform", False, True), (True, "gaussian", False, True), (True, "uniform", False, False),
                (True, "gaussian", True, False)]
ENGINE_IDS = ["dae_gaussian", "dae_uniform_draw", "cdae_x_gaussian_draw", "cdae_x_uniform", "cdae_a_gaussian"]
CFG = dict(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4)


@pytest.mark.parametrize("conditional,noise,enc_input,draw", ENGINE_CASES, ids=ENGINE_IDS)
def test_engine_replay_equals_eager_through_the_ramp(conditional, noise, enc_input, draw):
    B, S, ns, n = (5, 6, 2, 6) if conditional else (15, 1, 4, 6)         # N = 60: a partial 64-row tile
    cfg = net.DaeConfig(nsigma=ns, **CFG)
    data, runs = batches(conditional, n, B, S), []
    for graph in (True, False):
        net.manual_seed(77)
        eng = engine(conditional, fresh(conditional, noise, enc_input), cfg, B, S, graph=graph, draw_form=draw)
        assert eng.plain and eng.recon and eng.draw_form == draw and eng.noise_id == NOISE[noise] and eng.N == 60
        trace = []
        for i, batch in enumerate(data):
            eng.step(*batch)
            trace += [eng._net.flat_params().clone(), eng.loss.clone(), eng.xbar.clone(), eng.target.clone(), eng.eps.clone()] + [b.clone() for b in eng.opt.buffers()]
            st = eng.stats()
            assert set(st) == {"loss", "sigma"} and st["sigma"] == sigma32(cfg, i) and np.isfinite(st["loss"])
            assert torch.equal(eng.sigma, torch.ones(eng.N, device="cuda"))
            if noise == "uniform":
                assert 0.0 <= float(eng.eps.min()) and float(eng.eps.max()) < 1.0
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        runs.append(trace + [eng.state.clone()])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs)), "replayed != eager"
    per = 5 + len(eng.opt.buffers())
    losses = torch.cat(runs[0][1::per][:n])
    assert torch.isfinite(losses).all() and len(set(losses.tolist())) == n           # fresh noise every step
    assert runs[0][-1][:2].tolist() == [STRIDE * (n + 1), n + 1]
    # the two launch forms give the same bits: the same run with the other form
    net.manual_seed(77)
    other = engine(conditional, fresh(conditional, noise, enc_input), cfg, B, S, graph=False, draw_form=not draw)
    for batch in data:
        other.step(*batch)
    assert torch.equal(other._net.flat_params(), runs[1][-1 - per]) and torch.equal(other.state, runs[1][-1])
    # score() is the module's glogprob at the block's sigma (the coming step's), or at std=
    s = other.state[3:].view(torch.float32)[0].item()
    assert s == sigma32(cfg, n)
    g = torch.Generator().manual_seed(1)
    if conditional:
        lat, ctx, mean = torch.randn(3, 7, 2, generator=g).cuda(), torch.randn(3, 3, generator=g).cuda(), torch.randn(3, 2, generator=g).cuda()
        u = 1.5 * (lat - mean[:, None, :])
        for std, got in ((s, other.score(lat, ctx, mean)), (0.7, other.score(lat, ctx, mean, std=0.7))):
            assert got.shape == (3, 7, 2) and torch.equal(got, other.cdae.glogprob(u, ctx[:, None, :].expand(3, 7, 3), std))
    else:
        pts = torch.randn(100, 2, generator=g).cuda()
        assert torch.equal(other.score(pts), other.dae.glogprob(pts, s)) and torch.equal(other.score(pts, std=0.7), other.dae.glogprob(pts, 0.7))
        with pytest.raises(ValueError, match="takes std="):
            other.score(pts, torch.zeros(100, device="cuda"))


@pytest.mark.parametrize("conditional", [False, True], ids=["dae", "cdae_x"])
@pytest.mark.parametrize("noise", ["gaussian", "uniform"])
def test_engine_follows_the_recorded_trajectory(golden_dir, conditional, noise):
    """The reference's loop on the fixture's samples and draws: every parameter after every step against its fp32 run, and no further from its
    float64 run than max(2 x the fp32 reference's own distance, 2e-6) - score_gpu_checks.check_recorded_trajectory's criterion."""
    fx = load(os.path.join(golden_dir, f"recon_{'cdae' if conditional else 'dae'}_traj_{noise}.npz"))
    c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
    B, ns, d, h, nl, act, steps = int(c["B"]), int(c["nsigma"]), int(c["d"]), int(c["h"]), int(c["L"]), str(c["act"]), int(c["steps"])
    cfg = net.DaeConfig(sigma_max=float(c["sigma_max"]), sigma_min=float(c["sigma_min"]), sigma_annealing=int(c["sigma_annealing"]), nsigma=ns, lr=float(c["lr"]))
    kw = dict(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act, noise_type=noise)
    m = net.MLPCDAE(context_dim=int(c["c"]), enc_input=False, **kw) if conditional else net.MLPDAE(**kw)
    m.load_state_dict(state_dict_of(fx))
    if conditional:
        eng, names = net.ArdaeCondScoreEngine(m.cuda(), cfg, B, int(c["S"]), std_scale=float(c["std_scale"])), ("latent", "ctx", "mean")
    else:
        eng, names = net.ArdaeScoreEngine(m.cuda(), cfg, B), ("x",)
    bad = []
    for s in range(steps):
        eng.step(*(torch.tensor(fx[f"{s}/{k}"]).cuda() for k in names), noise={"eps": torch.tensor(fx[f"{s}/eps"]).cuda()})
        st = eng.stats()
        assert st["sigma"] == float(np.float32(float(fx[f"{s}/sigma"])))
        assert abs(st["loss"] - float(fx[f"{s}/loss"])) <= LOSS_TOL * abs(float(fx[f"{s}/loss"])), (s, st["loss"])
        for n, q in eng._net.named_parameters():
            p32, p64 = fx[f"{s}/p/{n}"], fx[f"{s}/p_f64/{n}"]
            e32, e64, ref64 = rel(q.detach().cpu(), p32), rel(q.detach().cpu(), p64), rel(p32, p64)
            print(f"{noise} step {s} {n}: to fp32 reference {e32:.2e}, to float64 {e64:.2e} (fp32 reference to float64 {ref64:.2e})")
            if e32 > TENSOR_TOL or e64 > max(2 * ref64, 2e-6):
                bad.append((s, n, e32, e64, ref64))
    assert not bad, bad


@pytest.mark.parametrize("conditional,noise,enc_input,draw", ENGINE_CASES[:4], ids=ENGINE_IDS[:4])
def test_engine_resumes_bit_identically(conditional, noise, enc_input, draw):
    """state_dict() after step 3 into a fresh engine under another library seed: steps 4 - 6 leave what the uninterrupted run leaves."""
    B, S, ns, n, at = (5, 6, 2, 6, 3) if conditional else (15, 1, 4, 6, 3)
    cfg = net.DaeConfig(nsigma=ns, **CFG)
    data, runs = batches(conditional, n, B, S), []
    for resumed in (False, True):
        net.manual_seed(77)
        eng = engine(conditional, fresh(conditional, noise, enc_input), cfg, B, S, draw_form=draw)
        losses = []
        for i, batch in enumerate(data):
            if resumed and i == at:
                sd = eng.state_dict()
                net.manual_seed(1)                                 # the checkpoint, not the process, carries the RNG state
                eng = engine(conditional, fresh(conditional, noise, enc_input, seed=5), cfg, B, S, draw_form=draw)
                eng.load_state_dict(sd)
                assert eng._graph is None and (eng.step_count, eng.opt.steps) == (at, at)
                assert list(sd) == [eng._NET, "optimizer", "engine"]
            eng.step(*batch)
            assert eng.stats()["sigma"] == sigma32(cfg, i)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        runs.append([eng._net.flat_params().clone(), eng.state.clone(), eng.xbar.clone(), torch.cat(losses)[at:]] + [b.clone() for b in eng.opt.buffers()])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the resumed run drifted"
    assert torch.isfinite(runs[0][3]).all() and len(set(runs[0][3].tolist())) == n - at


@pytest.mark.parametrize("conditional", [False, True], ids=["dae", "cdae"])
def test_engine_refuses_bad_noise_before_any_launch(conditional):
    B, S, ns = (4, 8, 2) if conditional else (16, 1, 4)
    eng = engine(conditional, fresh(conditional, "uniform"), net.DaeConfig(nsigma=ns, **CFG), B, S)
    good = batches(conditional, 1, B, S)[0]
    N = eng.N
    for bad in (torch.zeros(N // 2, 2, device="cuda"), torch.zeros(N, 2), torch.zeros(N, 3, device="cuda")):
        with pytest.raises(ValueError, match="eps must be"):
            eng.step(*good, noise={"eps": bad})
    with pytest.raises(ValueError, match="computes sigma on the device"):
        eng.step(*good, sigma=0.5)
    with pytest.raises(ValueError, match=f"batch_size={B}"):
        eng.step(good[0][:B - 1], *good[1:])
    assert eng.step_count == 0 and eng.opt.steps == 0 and eng.state[:2].tolist() == [STRIDE, 1]
    with pytest.raises(TypeError, match="(?s)DaeConfig.*ScoreConfig"):
        engine(conditional, fresh(conditional, "gaussian"), net.ScoreConfig(), B, S)
