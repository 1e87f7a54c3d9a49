"""Energy-function fitting on the device: one whole iteration of notebooks/ardae_fit.ipynb as ONE captured unit.

An iteration is `num_dae_updates` AR-DAE updates, each on a fresh sample of the implicit generator, then one generator update whose
output gradient is (alpha dE/dx + score(x, sigma = 0)) / B: the energy pulls the samples to the modes, the AR-DAE score - the gradient
of the sampler's log-density - keeps them spread.  No autograd, no host synchronisation: the energy weight alpha (annealed), the
generator's learning rate (StepLR) and Adam's coefficients are recomputed ON THE DEVICE by `ardae_fit_state_advance`, so the captured
graph replays with the right values; nothing of it is a frozen kernel argument.
"""
from dataclasses import dataclass

import torch

from . import _lib as L
from . import energy as E
from . import rng
from .engine import annealing_func
from .engine_common import RNG_STRIDE, CaptureLadder, bump_versions, check_tensor, rebuild_step_state
from .modules import Generator
from .score_engine import ArdaeScoreEngine, ScoreConfig

FIT_STATE_WORDS = L.CONSTANTS["ARDAE_FIT_STATE_BYTES"] // 8          # the block as int64 words; floats 8 .. 11 are its tail
_TAIL = L.CONSTANTS["ARDAE_STEP_STATE_BYTES"] // 4


@dataclass
class FitConfig:
    """The constants of notebooks/ardae_fit.ipynb."""
    energy: object = "energy_func4"   # 'energy_func1' .. 'energy_func4', 'normal_energy_func', or the net.energy callable itself
    num_dae_updates: int = 2          # AR-DAE updates per generator update
    nsigma: int = 10                  # `num_sigma`: noise levels per sample
    delta: float = 0.1                # sigma = delta * randn per row
    lr: float = 1e-3                  # both optimisers' (d_lr: the AR-DAE's, if it differs)
    m_beta1: float = 0.5              # torch.optim.Adam(lr, betas=(0.5, 0.999)) for the generator
    lr_step_size: int = 5000          # StepLR(step_size=5000, gamma=0.5, min_lr=1e-10) on it (utils/lr_scheduler.py), stepped per iteration
    lr_gamma: float = 0.5
    lr_min: float = 1e-10
    alpha_init: float = 0.01          # alpha = annealing_func(0.01, 1.0, 20000, iteration)  (utils/msc.py:53-55); alpha_annealing None: alpha_fin
    alpha_fin: float = 1.0
    alpha_annealing: object = 20000
    d_optimizer: str = "rmsprop"      # torch.optim.RMSprop(lr, momentum=0.5) for the AR-DAE (ScoreConfig's choices)
    d_momentum: float = 0.5
    d_beta1: float = 0.5
    d_lr: object = None               # None: lr
    energy_mu: float = 0.0            # normal_energy_func's mu / logvar
    energy_logvar: float = 0.0

    def __post_init__(self):
        E.kind_of(self.energy)
        if not 1 <= int(self.num_dae_updates) < RNG_STRIDE:
            raise ValueError(f"num_dae_updates must be in 1 .. {RNG_STRIDE - 1} (one Philox offset per generator sample of an "
                             f"iteration), got {self.num_dae_updates}")
        if int(self.nsigma) < 1:
            raise ValueError(f"nsigma must be positive, got {self.nsigma}")
        if int(self.lr_step_size) < 1 or not float(self.lr) > 0 or not float(self.lr_gamma) > 0 or float(self.lr_min) < 0:
            raise ValueError(f"bad learning-rate schedule: lr={self.lr}, lr_step_size={self.lr_step_size}, lr_gamma={self.lr_gamma}, lr_min={self.lr_min}")
        if self.alpha_annealing is not None and int(self.alpha_annealing) < 1:
            raise ValueError(f"alpha_annealing must be a positive number of iterations or None, got {self.alpha_annealing}")
        if not 0.0 <= float(self.m_beta1) < 1.0:
            raise ValueError(f"m_beta1 must be in [0, 1), got {self.m_beta1}")


def step_lr(cfg, iteration):
    """The generator's learning rate at `iteration` (0-based): StepLR.get_lr with last_epoch = iteration (utils/lr_scheduler.py)."""
    return max(cfg.lr_min, cfg.lr * cfg.lr_gamma ** (iteration // cfg.lr_step_size))


def alpha_at(cfg, iteration):
    return annealing_func(cfg.alpha_init, cfg.alpha_fin, cfg.alpha_annealing, iteration)


class ArdaeFitEngine:
    """`step()`: num_dae_updates x (draw z, generator forward, one AR-DAE update on that sample - ArdaeScoreEngine's body), then draw,
    forward, score at sigma 0, fused energy seed, generator backward, torch-style Adam, re-pack, fit-state advance - on ONE stream as ONE
    linear HIP graph, captured at the third call and replayed afterwards (replayed == eager bit for bit).
    `step(noise={'z': [U + 1, B, z_dim], 'sigma': [U, B * nsigma], 'eps': [U, B * nsigma, d]})` runs the same launches eagerly on injected
    draws.  `stats()` is the only synchronising call.

    Philox offsets: the generator's sample u of iteration i (0-based) is the draw Z_STREAM + RNG_STRIDE (i + 1) + u; the embedded AR-DAE
    update k (1-based) uses RNG_STRIDE k + {0, 1} as in ArdaeScoreEngine; host-side draws (`sample`, net.rng) have the top bit set."""

    RNG_STRIDE = RNG_STRIDE
    Z_STREAM = 1 << 62

    def __init__(self, generator, dae, cfg: FitConfig, batch_size, graph=True):
        if not isinstance(generator, Generator):
            raise TypeError("ArdaeFitEngine drives net.Generator")
        generator._require_gpu()
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        self.gen, self.dae, self.cfg = generator, dae, cfg
        self.B, self.U, self.d, self.zd = int(batch_size), int(cfg.num_dae_updates), generator.input_dim, generator.z_dim
        self.kind = E.kind_of(cfg.energy)
        if E.KINDS["energy_func1"] <= self.kind <= E.KINDS["energy_func4"] and self.d != 2:
            raise ValueError(f"energy_func1 .. energy_func4 are defined on 2 dimensions, the generator has input_dim={self.d}")
        # the AR-DAE half: ArdaeScoreEngine's buffers, optimiser and body; its own graph stays off - the body runs inside this engine's
        self.score = ArdaeScoreEngine(dae, ScoreConfig(delta=cfg.delta, nsigma=cfg.nsigma, lr=cfg.lr if cfg.d_lr is None else cfg.d_lr,
                                                       optimizer=cfg.d_optimizer, beta1=cfg.d_beta1, momentum=cfg.d_momentum), self.B, graph=False)
        if self.score.d != self.d:
            raise ValueError(f"the score network has input_dim={self.score.d}, the generator {self.d}")
        self.dev = generator._flat.device
        if self.score.dev != self.dev:
            raise ValueError(f"generator on {self.dev}, score network on {self.score.dev}")
        self._ladder = CaptureLadder(self.dev, graph)
        self.net = generator._net
        f = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
        B, d = self.B, self.d
        self.ws = f(L.query("ardae_gen_workspace_floats", *self.net, B))
        self.ws_score = f(L.query("ardae_cdae_workspace_floats", dae._desc, B, 1, 0))
        self.pk = f(L.query("ardae_gen_packed_floats", *self.net))
        self.z, self.x, self.sc, self.seed = f(B, self.zd), f(B, d), f(B, d), f(B, d)
        self._zero = torch.zeros(B, device=self.dev)
        self.model_loss = f(1)
        self.partial = f(L.query("ardae_energy_partial_floats", B))
        self.grads = torch.zeros_like(generator._flat)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(generator._flat), torch.zeros_like(generator._flat)
        self.state = torch.zeros(FIT_STATE_WORDS, dtype=torch.int64, device=self.dev)
        self.fused_front = L.debug_knob("ARDAE_FUSED_GEN_FRONT", "1") != "0" and bool(L.query("ardae_gen_draw_fused_ok", *self.net))
        self._sample_ws = {}
        self.step_count = 0
        self._advance()                # the fit state always describes the COMING iteration
        self.repack()

    _graph = property(lambda self: self._ladder.graph)          # None until the iteration has been captured
    use_graph = property(lambda self: self._ladder.on, lambda self, on: setattr(self._ladder, "on", bool(on)))

    # ------------------------------------------------------------------------------------------------------------
    @classmethod
    def z_offset_add(cls, u):
        """What the launch of generator sample u adds to the fit state's Philox base offset (the one place that defines it)."""
        return cls.Z_STREAM + int(u)

    @classmethod
    def philox_offsets(cls, iteration, num_dae_updates):
        """Every Philox offset iteration `iteration` (0-based) draws with: {'z': U + 1 offsets, 'dae': U (sigma, eps) pairs}."""
        U = int(num_dae_updates)
        base = cls.RNG_STRIDE * (iteration + 1)
        return {"z": [cls.z_offset_add(u) + base for u in range(U + 1)],
                "dae": [(cls.RNG_STRIDE * (iteration * U + u + 1), cls.RNG_STRIDE * (iteration * U + u + 1) + 1) for u in range(U)]}

    def _advance(self):
        c = self.cfg
        L.call("ardae_fit_state_advance", self.state, self.RNG_STRIDE, float(c.lr), float(c.m_beta1), 0.999, int(c.lr_step_size), float(c.lr_gamma),
               float(c.lr_min), float(c.alpha_init), float(c.alpha_fin), -1 if c.alpha_annealing is None else int(c.alpha_annealing))

    def repack(self):
        L.call("ardae_gen_pack", *self.net, self.gen._flat, self.pk)
        self.score.repack()

    def _sample_into_x(self, u, z):
        """x = generator(z_u): the draw u of this iteration, or the injected batch."""
        flat, seed = self.gen._flat, rng.get_state()["seed"]
        if z is None and self.fused_front:
            L.call("ardae_gen_draw_forward", *self.net, flat, self.pk, self.B, seed, self.z_offset_add(u), self.state, self.z, self.ws, self.ws.numel(), self.x)
            return
        if z is None:
            L.call("ardae_philox_normal_at", self.z, self.B * self.zd, seed, self.z_offset_add(u), self.state, 0)
        else:
            self.z.copy_(z)
        L.call("ardae_gen_forward", *self.net, flat, self.pk, self.z, self.B, self.ws, self.ws.numel(), self.x)

    def _body(self, noise):
        sc, c = self.score, self.cfg
        for u in range(self.U):
            self._sample_into_x(u, None if noise is None else noise["z"][u])
            if noise is not None:           # into the score engine's own buffers, as its step(noise=...) does
                sc.sigma.copy_(noise["sigma"][u].reshape(-1))
                sc.eps.copy_(noise["eps"][u].reshape(sc.N, self.d))
            sc._body(self.x, noise is None)
        self._sample_into_x(self.U, None if noise is None else noise["z"][self.U])
        L.call("ardae_cdae_score", self.dae._desc, self.dae._flat, sc.pk, self.x, self._zero, None, self.B, 1, self.ws_score, self.ws_score.numel(), self.sc)
        L.call("ardae_energy_seed", self.kind, self.x, self.sc, self.B, self.d, float(c.energy_mu), float(c.energy_logvar), 0.0, self.state, self.seed,
               self.model_loss, self.partial)
        L.call("ardae_gen_backward", *self.net, self.gen._flat, self.pk, self.z, self.seed, self.B, self.ws, self.ws.numel(), self.grads)
        L.call("ardae_adam_torch_step_dev", self.gen._flat, self.grads, self.exp_avg, self.exp_avg_sq, self.gen._flat.numel(), float(c.m_beta1), 0.999,
               1e-8, self.state)
        L.call("ardae_gen_pack", *self.net, self.gen._flat, self.pk)
        self._advance()

    def _check_noise(self, noise):
        N = self.B * int(self.cfg.nsigma)
        want = {"z": (self.U + 1, self.B, self.zd), "sigma": (self.U, N), "eps": (self.U, N, self.d)}
        if not isinstance(noise, dict) or set(noise) != set(want):
            raise ValueError(f"step(noise): expected a dict with the keys {sorted(want)}")
        for k, shape in want.items():
            check_tensor(noise[k], f"step(noise): {k}", self.dev, shape=shape)

    def step(self, noise=None):
        """One iteration of ardae_fit.ipynb."""
        if noise is not None:
            self._check_noise(noise)
        self._ladder.run(lambda: self._body(noise), eager=noise is not None)
        self.step_count += 1
        for _ in range(self.U):
            self.score._count_step()
        bump_versions(self.gen)

    def sample(self, n):
        """n generator samples [n, input_dim] with the current weights; draws from the host Philox stream, touches no training state."""
        n = int(n)
        if n < 1:
            raise ValueError(f"sample(n): n must be positive, got {n}")
        ws = self._sample_ws.get(n)
        if ws is None:
            ws = self._sample_ws[n] = torch.empty(L.query("ardae_gen_workspace_floats", *self.net, n), device=self.dev)
        z = rng.normal((n, self.zd), self.dev)
        x = torch.empty(n, self.d, device=self.dev)
        L.call("ardae_gen_forward", *self.net, self.gen._flat, self.pk, z, n, ws, ws.numel(), x)
        return x

    def stats(self):
        """Host copy of the last iteration's scalars (the only synchronising call): the generator's loss (mean energy), the last AR-DAE
        loss, and the alpha / lr that iteration used, as the device computed them."""
        v = torch.cat([self.model_loss, self.score.loss, self.state.view(torch.float32)[_TAIL + 2:_TAIL + 4]]).tolist()
        return dict(model_loss=v[0], dae_loss=v[1], alpha=v[2], lr=v[3])

    # ------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """Generator, torch.optim.Adam's state_dict() layout for it plus the schedule's last_epoch, the AR-DAE and its optimiser, and the
        RNG state: everything a resumed run needs to continue bit-identically."""
        c, t, dae = self.cfg, self.step_count, self.score.state_dict()
        views = list(zip(self.gen.param_views(self.exp_avg), self.gen.param_views(self.exp_avg_sq)))
        adam = {i: {"step": torch.tensor(float(t)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()} for i, (m, v) in enumerate(views)} if t else {}
        group = {"lr": step_lr(c, t), "betas": (float(c.m_beta1), 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "initial_lr": float(c.lr), "params": list(range(len(views)))}
        return {"generator": {k: v.clone() for k, v in self.gen.state_dict().items()},
                "optimizer": {"state": adam, "param_groups": [group]},
                "scheduler": {"step_size": int(c.lr_step_size), "gamma": float(c.lr_gamma), "min_lr": float(c.lr_min), "base_lrs": [float(c.lr)],
                              "last_epoch": t, "_last_lr": [step_lr(c, t)]},
                "dae": dae["dae"], "dae_optimizer": dae["optimizer"],
                "engine": {"step_count": t, "dae_steps": dae["engine"]["step_count"], "rng_seed": dae["engine"]["rng_seed"],
                           "rng_host_offset": dae["engine"]["rng_host_offset"], "fit_state": self.state.cpu().clone(),
                           "dae_step_state": dae["engine"]["step_state"]}}

    def load_state_dict(self, sd):
        """Inverse of state_dict().  Without the "engine" entry (a checkpoint assembled from torch objects) the iteration count is the
        schedule's last_epoch and the device blocks are rebuilt for it: the run continues with Philox offsets it has not used."""
        self.gen.load_state_dict(sd["generator"])
        eng = sd.get("engine")
        t = int(sd["scheduler"]["last_epoch"]) if eng is None else int(eng["step_count"])
        steps = {int(st["step"]) for st in sd["optimizer"]["state"].values()}
        if steps - {t}:
            raise ValueError(f"the generator's Adam state is at step {sorted(steps)}, the schedule at {t}: the engine keeps one iteration count")
        with torch.no_grad():
            for buf, key in ((self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
                buf.zero_()
                for i, v in enumerate(self.gen.param_views(buf)):
                    if i in sd["optimizer"]["state"]:
                        v.copy_(sd["optimizer"]["state"][i][key])
        # the AR-DAE half is the score engine's own checkpoint under this dictionary's keys (it restores the RNG state too)
        dae = {"dae": sd["dae"], "optimizer": sd["dae_optimizer"]}
        if eng is not None:
            dae["engine"] = {"step_count": eng["dae_steps"], "rng_seed": eng["rng_seed"], "rng_host_offset": eng["rng_host_offset"],
                             "step_state": eng["dae_step_state"]}
        self.score.load_state_dict(dae, default_steps=t * self.U)
        self.step_count = t
        if eng is not None:
            self.state.copy_(eng["fit_state"].to(self.dev))
        else:
            rebuild_step_state(self.state, t, self.RNG_STRIDE, self._advance)
        self._ladder.reset()                     # parameters were rewritten outside of the captured iteration
        bump_versions(self.gen)
        self.repack()
