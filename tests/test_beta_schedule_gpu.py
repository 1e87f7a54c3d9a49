"""--beta-init / --beta-annealing on the device (ivae_ardae.py:202-203,704; utils/msc.py:53-55): `ardae_train_state_advance` writes the
coming step's beta and entropy-seed factor into the last 8 bytes of the step block, the `_dev` entry points read them there, and
`ArdaeEngine` with `TrainConfig(beta_init=, beta_annealing=)` captures its step once and replays it while beta moves.

Everything here is an equality of bits: the device forms beta and the seed factor with the host's own double operations, and a `_dev`
twin runs the value form's kernels with the float loaded through a pointer."""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O
from test_engine_gpu import CASES, build, train_config

pytestmark = pytest.mark.gpu

MC = O.ModelCfg("mnist", 24, 10, 64, 8, 2, "softplus")      # the tiny shape of test_engine_beta_annealing_under_graph_mode
CC = O.CdaeCfg("grad", 8, 8, 64, 3)
SCHED = dict(beta=1.0, beta_init=0.1, beta_annealing=6)
STRIDE = net.ArdaeEngine.RNG_STRIDE


def sched_beta(i, init=0.1, fin=1.0, ann=6):
    return net.annealing_func(init, fin, ann, i)


def block_floats(state):
    """(beta, seed_scale) of a step block [4] int64 - bytes 24..31."""
    v = state.cpu().numpy().view(np.float32)
    return v[6], v[7]


# ---- 1. the state kernel -----------------------------------------------------------------------------------------------------------
def _advance_and_check(state, twin, init, fin, ann, std_scale, rows, nsteps):
    lr, b1 = 1e-3, 0.9
    snaps, twins = [], []
    for _ in range(nsteps):
        L.call("ardae_train_state_advance", state, STRIDE, lr, b1, 0.999, init, fin, ann, std_scale, rows)
        L.call("ardae_step_state_advance", twin, STRIDE, lr, b1, 0.999)
        snaps.append(state.clone())
        twins.append(twin.clone())
    snaps, twins = torch.stack(snaps).cpu().numpy(), torch.stack(twins).cpu().numpy()
    assert np.array_equal(snaps[:, :3], twins[:, :3])                  # the first 24 bytes: exactly ardae_step_state_advance's
    assert not twins[:, 3].any()                                       # ... which leaves the last 8 alone
    for row in snaps:
        t = int(row[1])
        beta64 = net.annealing_func(init, fin, None if ann < 0 else ann, t - 1)
        got = row.view(np.float32)[6:8]
        want = (np.float32(beta64), np.float32(std_scale * beta64 / float(rows)))
        assert got[0] == want[0] and got[1] == want[1], (init, fin, ann, std_scale, rows, t, tuple(got), want)
    return int(snaps[-1][1])


@pytest.mark.parametrize("init,fin,ann", [(0.1, 1.0, 3), (1e-4, 1.0, 50000), (1.0, 1.0, -1), (2.0, 0.5, 7)])
def test_train_state_advance_matches_the_host_bit_for_bit(init, fin, ann):
    for std_scale in (1.0, 100.0):
        for rows in (4, 128):
            state = torch.zeros(4, dtype=torch.int64, device="cuda")
            twin = torch.zeros_like(state)
            nsteps = 20 if ann == 50000 else max(ann, 0) + 3
            assert _advance_and_check(state, twin, init, fin, ann, std_scale, rows, nsteps) == nsteps
            if ann == 50000:      # across the end of the ramp: the blocks pre-set so that the next t is 49 998 .. 50 002
                for blk in (state, twin):
                    blk.zero_()
                    blk[0], blk[1] = STRIDE * 49997, 49997
                assert _advance_and_check(state, twin, init, fin, ann, std_scale, rows, 5) == 50002


def test_train_state_advance_refuses_a_zero_ramp():
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        L.call("ardae_train_state_advance", state, STRIDE, 1e-3, 0.9, 0.999, 0.1, 1.0, 0, 1.0, 4)
    with pytest.raises(ValueError):
        L.call("ardae_train_state_advance", state, STRIDE, 1e-3, 0.9, 0.999, 0.1, 1.0, 3, 1.0, 0)


# ---- 2. the twins against the value forms ------------------------------------------------------------------------------------------
def _block(beta, seed_scale):
    host = np.zeros(4, dtype=np.int64)
    host.view(np.float32)[6:8] = (beta, seed_scale)
    return torch.from_numpy(host).cuda()


def _tiny_model():
    model, _ = build(MC, CC)
    model.load_state_dict(O.init_params(O.model_param_spec(MC), 0, O.model_init_special(MC)))
    return model.to("cuda")


@pytest.mark.parametrize("nz", [1, 3])
def test_dev_twins_equal_the_value_forms(nz):
    B, beta, seed = 4, float(np.float32(0.37)), float(np.float32(12.5 * 0.37))
    model = _tiny_model()
    md, flat, pk = model._desc, model._flat, model._packed_weights()
    gen = torch.Generator().manual_seed(5)
    x = torch.bernoulli(torch.full((B, MC.input_dim), 0.3), generator=gen).cuda()
    nv = torch.randn(B * nz, model._noise_width, generator=gen).cuda()
    g = torch.randn(B * nz, MC.z_dim, generator=gen).cuda()
    state = _block(beta, seed)
    f = lambda *s: torch.zeros(*s, device="cuda")

    def run(dev, split):
        ws = f(L.query("ardae_model_workspace_floats", md, B, nz, 1))
        z, losses, grads = f(B * nz, MC.z_dim), f(3), f(flat.numel())
        sfx, b, s = ("_dev", state, state) if dev else ("", beta, seed)
        L.call("ardae_model_vae_forward" + sfx, md, flat, pk, x, nv, B, nz, b, ws, ws.numel(), z, losses)
        if split:
            L.call("ardae_model_vae_backward_decoder" + sfx, md, flat, pk, x, nv, B, nz, b, 1.0, ws, ws.numel())
            L.call("ardae_model_vae_backward_sampler" + sfx, md, flat, pk, x, nv, B, nz, g, s, ws, ws.numel(), grads, 0.0)
        else:
            L.call("ardae_model_vae_backward" + sfx, md, flat, pk, x, nv, B, nz, b, 1.0, g, ws, ws.numel(), grads, 0.0)
        return z, losses, grads

    for split in (False, True):
        want, got = run(False, split), run(True, split)
        assert float(want[2].abs().sum()) > 0 and float(want[1][0]) != float(want[1][1])      # beta and the seed did enter
        for a, b, what in zip(want, got, ("z", "losses", "grads")):
            assert torch.equal(a, b), (what, split)


@pytest.mark.parametrize("n", [4 * 8, 7, 1027])
def test_seed_scale_kernel_equals_the_host_scalar_multiply(n):
    seed = float(np.float32(1e4 * 0.37 / 12.0))
    state = _block(0.37, seed)
    base = torch.randn(n + 1, generator=torch.Generator().manual_seed(n)).cuda()
    for off in (0, 1):                      # 16-byte aligned, and 4 bytes past it: the scalar head
        g = base.clone()[off:off + n]
        want = base[off:off + n] * seed
        L.call("ardae_seed_scale_dev", g, n, state)
        assert torch.equal(g, want), (n, off)


def test_log_scalars_twin_writes_the_blocks_beta():
    state = _block(0.37, 1.0)
    state[1] = 3                            # iter 3 -> ring slot 2
    loss_c, losses, std_b = torch.ones(1, device="cuda"), torch.arange(3.0, device="cuda"), torch.rand(4, device="cuda")
    rings = [torch.zeros(4, L.LOG_RECORD_FLOATS, device="cuda") for _ in range(2)]
    L.call("ardae_log_scalars", loss_c, losses, std_b, 4, float(np.float32(0.37)), 1e-4, state, rings[0], 4)
    L.call("ardae_log_scalars_dev", loss_c, losses, std_b, 4, state, 1e-4, state, rings[1], 4)
    assert torch.equal(rings[0], rings[1]) and float(rings[1][2, 4]) == float(np.float32(0.37))


# ---- 3 - 5. the engine ---------------------------------------------------------------------------------------------------------------
def _images(mc, n, B=4, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [torch.bernoulli(torch.full((B, mc.input_dim), 0.3), generator=gen).cuda() for _ in range(n)]


def _engine(mc, cc, cfg, graph, B=4):
    model, cdae = build(mc, cc)
    model.load_state_dict(O.init_params(O.model_param_spec(mc), 0, O.model_init_special(mc)))
    cdae.load_state_dict(O.init_params(O.cdae_param_spec(cc), 1))
    model, cdae = model.to("cuda"), cdae.to("cuda")
    return net.ArdaeEngine(model, cdae, cfg, batch_size=B, graph=graph), model, cdae


def _run(eng, xs, first, last, betas=None, captured=None):
    n = len(xs)
    for t in range(first, last):
        eng.step(xs[t % n], xs[(t + 3) % n], **({} if betas is None else {"beta": betas[t]}))
        if captured is not None:
            captured.append(eng._graph is not None)
    torch.cuda.synchronize()


def _params(model, cdae):
    return model.flat_params().clone(), cdae.flat_params().clone()


def test_engine_replays_through_the_schedule():
    xs = _images(MC, 8)
    betas = [sched_beta(t) for t in range(8)]
    assert betas[0] == 0.1 and betas[2] < betas[3] < betas[6] == betas[7] and np.float32(betas[7]) == 1.0      # (0.9999999999999999 in double)
    outs, captured = [], []
    for graph in (True, False):
        net.manual_seed(17)
        eng, model, cdae = _engine(MC, CC, net.TrainConfig(nz_cdae=8, **SCHED), graph)
        log = net.ScalarLog(eng, capacity=16) if graph else None
        with pytest.raises(ValueError):
            eng.step(xs[0], xs[3], beta=0.5)              # two sources of truth
        _run(eng, xs, 0, 8, captured=captured if graph else None)
        outs.append(_params(model, cdae))
        if graph:
            plan = eng.plan_summary()
            logged = [np.float32(r["train/model/beta/step"]) for r in log.drain()]
        else:
            assert eng._graph is None
    # the schedule's ladder: an eager first step, the capture at the next one, replays after - so the graph exists after the step at
    # index 2 while beta is still moving (0.4 of 1.0); a caller-fed beta would keep the engine eager until index 7
    assert captured == [False] + [True] * 7
    assert logged == [np.float32(b) for b in betas]
    # a schedule-free engine fed the same betas by the caller, eagerly: today's annealing phase
    net.manual_seed(17)
    eng, model, cdae = _engine(MC, CC, net.TrainConfig(nz_cdae=8), False)
    _run(eng, xs, 0, 8, betas=betas)
    outs.append(_params(model, cdae))
    for other in outs[1:]:
        assert torch.equal(outs[0][0], other[0]) and torch.equal(outs[0][1], other[1])
    # the same graphs as a constant-beta step's (the log's launch aside: it joins the last unit)
    net.manual_seed(17)
    eng, _, _ = _engine(MC, CC, net.TrainConfig(nz_cdae=8), True)
    _run(eng, xs, 0, 3)
    assert eng.plan_summary() is not None and plan == eng.plan_summary()


def test_teacher_forced_step_and_phase_calls_read_the_block():
    """noise= and the direct phase calls take beta from the block too: one injected step equals the caller-fed one, bit for bit."""
    B, tc = 4, O.TrainCfg(nz_cdae=8)
    gen = torch.Generator().manual_seed(9)
    x1, x2 = (torch.bernoulli(torch.full((B, MC.input_dim), 0.3), generator=gen).cuda() for _ in range(2))
    noise = {k: v.cuda().contiguous() for k, v in O.draw_step_noise(MC, tc, B, gen).items()}
    outs = []
    for cfg, kw in ((net.TrainConfig(nz_cdae=8, **SCHED), {}), (net.TrainConfig(nz_cdae=8), {"beta": sched_beta(0)})):
        eng, model, cdae = _engine(MC, CC, cfg, True)
        eng.step(x1, x2, noise=noise, **kw)
        eng.cdae_phase(x1, noise)
        if not kw:
            with pytest.raises(ValueError):
                eng.vae_phase(x2, noise, beta=0.3)
        eng.vae_phase(x2, noise, **({"beta": sched_beta(1)} if kw else {}))
        torch.cuda.synchronize()
        outs.append(_params(model, cdae) + (eng.losses_m.clone(),))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("name", ["tiny_auxmnist_grad", "resconv_b4_nz8"])
def test_non_split_families_replay_through_the_schedule(name):
    """The families whose backward is one call (the seed is scaled by `ardae_seed_scale_dev` first): the aux sampler with the hidden1a
    context, and the residual-conv model of the annealed recipes."""
    mc, cc, nz, _ = CASES[name]
    xs = _images(mc, 4)
    outs = []
    for graph in (True, False):
        net.manual_seed(17)
        eng, model, cdae = _engine(mc, cc, train_config(mc, nz, **SCHED), graph)
        assert not eng.split_backward
        _run(eng, xs, 0, 4)
        assert (eng._graph is not None) == graph
        outs.append(_params(model, cdae))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # ... and the eager run equals the caller-fed one
    net.manual_seed(17)
    eng, model, cdae = _engine(mc, cc, train_config(mc, nz), False)
    _run(eng, xs, 0, 4, betas=[sched_beta(t) for t in range(4)])
    assert torch.equal(outs[1][0], model.flat_params()) and torch.equal(outs[1][1], cdae.flat_params())


def test_checkpoint_resumes_the_schedule():
    xs = _images(MC, 8)
    cfg = lambda: net.TrainConfig(nz_cdae=8, **SCHED)
    net.manual_seed(17)
    eng, model, cdae = _engine(MC, CC, cfg(), True)
    _run(eng, xs, 0, 8)
    want = _params(model, cdae)

    net.manual_seed(17)
    eng, model, cdae = _engine(MC, CC, cfg(), True)
    _run(eng, xs, 0, 4)
    ck_m, ck_c = eng.model_checkpoint(), eng.cdae_checkpoint()
    assert block_floats(ck_m["engine"]["step_state"])[0] == np.float32(sched_beta(4))

    old = copy.deepcopy(ck_m)                  # a file written before the block carried beta
    old["engine"]["step_state"][3] = 0
    for ck in (ck_m, old):
        net.manual_seed(1)                     # the file's seed and offsets take over
        eng2, model2, cdae2 = _engine(MC, CC, cfg(), True)
        eng2.load_checkpoints(copy.deepcopy(ck), copy.deepcopy(ck_c))
        rows = eng2.B * eng2.cfg.nz_model          # the per-rank rows of the seed (ivae_ardae.py:834)
        assert block_floats(eng2.state) == (np.float32(sched_beta(4)), np.float32(eng2.cfg.std_scale * sched_beta(4) / float(rows)))
        assert torch.equal(eng2.state[:3], ck["engine"]["step_state"][:3].cuda())
        _run(eng2, xs, 4, 8)
        got = _params(model2, cdae2)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    ref = {k: v for k, v in ck_m.items() if k != "engine"}      # the reference loop's file: no engine entry, the block is rebuilt
    eng3, model3, cdae3 = _engine(MC, CC, cfg(), True)
    eng3.load_checkpoints(ref, copy.deepcopy(ck_c))
    assert eng3.step_count == 4 and int(eng3.state[1]) == 5
    assert block_floats(eng3.state)[0] == np.float32(net.annealing_func(0.1, 1.0, 6, 4))
    _run(eng3, xs, 4, 6)
    assert block_floats(eng3.state)[0] == np.float32(sched_beta(6)) and bool(torch.isfinite(model3.flat_params()).all())


# ---- 6. two ranks ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    from ardae_amd import dist
    lo, hi = dist.shard_rows(4)
    xs = [x[lo:hi].contiguous() for x in _images(MC, 5)]
    res = {}
    for tag, cfg, graph, betas in (("sched", net.TrainConfig(nz_cdae=8, **SCHED), True, None),
                                   ("fed", net.TrainConfig(nz_cdae=8), False, [sched_beta(t) for t in range(5)])):
        net.manual_seed(17)
        eng, model, cdae = _engine(MC, CC, cfg, graph, B=hi - lo)
        _run(eng, xs, 0, 5, betas=betas)
        res[tag] = (model.flat_params().cpu(), cdae.flat_params().cpu(), eng.plan_summary())
    if rank == 0:
        torch.save(res, out)
    torch.distributed.destroy_process_group()


def test_two_ranks_replay_through_the_schedule(tmp_path):
    """B 2 per rank (gloo, both ranks on the one GPU): the seed factor is formed with the PER-RANK rows, every rank computes the same beta
    from the same t, and five replayed steps equal five eager steps with caller-fed betas."""
    out = str(tmp_path / "beta_dp.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out, weights_only=True)
    assert got["fed"][2] is None
    assert got["sched"][2] == ["graph:side", "graph:main", "allreduce", "graph:main", "graph:main", "allreduce", "graph:main"]
    assert torch.equal(got["sched"][0], got["fed"][0]) and torch.equal(got["sched"][1], got["fed"][1])
