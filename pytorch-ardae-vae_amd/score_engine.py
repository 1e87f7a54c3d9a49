"""Score networks outside the VAE loop: the update of an unconditional (notebooks/ardae_toy.ipynb, ardae_fit.ipynb, dae_toy.ipynb) or
conditional (ivae_ardae.py:743-779, on the caller's samples) score network as ONE captured unit.

`_ScoreEngine` holds what the two engines share - the network / config pairing, the buffers every update has, the optimiser and its step
block, noise intake, the tail of an update, the host bookkeeping, the plain kinds' stats() and the checkpoint; `ArdaeScoreEngine` and
`ArdaeCondScoreEngine` add their shapes, their extra buffers, the front of the update (which perturbation / fused launches run), `step`'s
batch checks, `score` and the AR kinds' stats().
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import rng
from .engine_common import RNG_STRIDE, CaptureLadder, _FlatOpt, bump_versions, check_batch, check_tensor, rebuild_step_state


@dataclass
class ScoreConfig:
    """Constants of the notebooks' AR-DAE update (ardae_toy.ipynb: delta 1, num_sigma 10, lr 5e-3; ardae_fit.ipynb: lr 1e-3)."""
    delta: float = 1.0            # sigma = delta * randn per row
    nsigma: int = 10              # noise levels per sample (`num_sigma`): a batch of B samples is B * nsigma rows
    lr: float = 1e-3
    optimizer: str = "rmsprop"    # sgd | adam | amsgrad | rmsprop (_FlatOpt).  "adam" is the reference's VENDORED Adam (utils/optim.py:
    beta1: float = 0.5            # epsilon before the bias correction), not the torch.optim.Adam the notebooks construct; for that one
    momentum: float = 0.5         # use the module path (MLPGradARDAE + torch.optim.Adam).  rmsprop and sgd coincide with torch's.


@dataclass
class DaeConfig:
    """Constants of notebooks/dae_toy.ipynb's training cell: one noise level per step, annealed linearly from sigma_max to sigma_min over
    sigma_annealing steps and computed on the device (ardae_dae_state_advance); torch.optim.Adam(lr=0.005)."""
    sigma_max: float = 5.0
    sigma_min: float = 0.05
    sigma_annealing: int = 4000   # steps of the ramp; 0 or below: the constant sigma_min
    nsigma: int = 10              # `num_sigma`: a batch of B samples is B * nsigma rows (each with its own eps)
    lr: float = 5e-3
    optimizer: str = "adam_torch"  # torch.optim.Adam, the notebook's (_FlatOpt; sgd | adam | amsgrad | rmsprop as for ScoreConfig)
    beta1: float = 0.9
    momentum: float = 0.0

    def __post_init__(self):
        if int(self.sigma_annealing) != self.sigma_annealing:
            raise ValueError(f"sigma_annealing must be a whole number of steps (got {self.sigma_annealing!r})")


def dae_sigma(sigma_max, sigma_min, sigma_annealing, step):
    """The noise level of 0-based step `step` (the notebook's i_ep), in the notebook's operation order; numpy.float32 of it is what
    ardae_dae_state_advance writes for t = step + 1."""
    if sigma_annealing <= 0:
        return float(sigma_min)
    perc = min((step + 1) / float(sigma_annealing), 1.0)
    return sigma_max * (1 - perc) + sigma_min * perc


class _ScoreEngine:
    """What ArdaeScoreEngine and ArdaeCondScoreEngine share.  A subclass names its network attribute (`_NET`, also the checkpoint key), its
    AR-DAE and plain ABI kinds and its refusal text, calls `_pair` and `_allocate` from its constructor, and writes `_front`, `step`,
    `score` and `_ar_stats`.

    The contract of an engine that embeds the update in a captured unit of its own (ArdaeFitEngine): `_body(*front)` ISSUES the launches of
    one update on the engine's buffers and does nothing else on the host; `_count_step()` is the host bookkeeping that follows each of
    them, outside the capture."""

    RNG_STRIDE = RNG_STRIDE
    _NET = _AR_KINDS = _PLAIN_KINDS = _DRIVES = _CHECKPOINT = None

    def _pair(self, net, cfg):
        """The network must be one of this engine's kinds and the config the one its family takes; nothing has touched the device yet."""
        net._require_gpu()
        kind = int(net._desc.kind)
        if kind not in self._AR_KINDS + self._PLAIN_KINDS:
            raise TypeError(self._DRIVES)
        self.plain = kind in self._PLAIN_KINDS
        # a reconstruction DAE (models/dae/mlp.py) shares its network kind with a residual one: the module says which it is
        self.recon = bool(getattr(net, "_recon", False))
        self.noise_id = net.NOISE[net.noise_type] if self.recon else 0
        if not isinstance(cfg, DaeConfig if self.plain else ScoreConfig):
            raise TypeError(f"{type(net).__name__} takes a {'DaeConfig' if self.plain else 'ScoreConfig'}, not a {type(cfg).__name__}: ScoreConfig "
                            "(a sigma draw per row) belongs to the AR-DAE networks, DaeConfig (one annealed sigma per step) to the plain DAEs")

    def _allocate(self, net, cfg, B, S, width, graph):
        """The buffers of an update on B * S rows of `width` values (self.N = B * S, in the factorisation the workspace is asked for), the
        optimiser and its step block - advanced once: it always describes the COMING step - and the packed weights."""
        setattr(self, self._NET, net)
        self._net, self.cfg = net, cfg
        self.dev = net._flat.device
        f = self._f
        self.ws = f(L.query("ardae_cdae_workspace_floats", net._desc, B, S, 1))
        self.xbar, self.sigma, self.eps = f(self.N, width), f(self.N), f(self.N, width)
        # a reconstruction DAE: eps holds the raw draw, and the loss layer reads (sigma = 1, target = -x) in the place of (sigma, eps)
        self.target = f(self.N, width) if self.recon else self.eps
        self.loss = f(1)
        self.grads = torch.zeros_like(net._flat)
        self.n_grad = net._flat.numel() - (1 if net._kind == "grad" else 0)     # neglogprob.fc.bias gets no gradient and keeps no state
        self.state = torch.zeros(4, dtype=torch.int64, device=self.dev)
        self.sched = (float(cfg.sigma_max), float(cfg.sigma_min), int(cfg.sigma_annealing)) if self.plain else None
        self.opt = _FlatOpt(cfg.optimizer, net._flat, self.n_grad, cfg.lr, cfg.beta1, cfg.momentum, state=self.state, dae=self.sched)
        self._ladder = CaptureLadder(self.dev, graph)
        self._score_ws = {}
        self.step_count = 0
        self.opt.advance(RNG_STRIDE)
        self.repack()

    def _f(self, *shape):
        """An uninitialised float32 buffer on the engine's device."""
        return torch.empty(*shape, device=self.dev, dtype=torch.float32)

    def repack(self):
        self._net._packed = None
        self.pk = self._net._packed_weights()

    _graph = property(lambda self: self._ladder.graph)          # None until the step has been captured
    use_graph = property(lambda self: self._ladder.on, lambda self, on: setattr(self._ladder, "on", bool(on)))

    def _refuse_sigma(self, sigma):
        if sigma is not None:
            raise ValueError(f"sigma={sigma!r}: " + (f"this engine computes sigma on the device (DaeConfig(sigma_max={self.cfg.sigma_max}, sigma_min="
                             f"{self.cfg.sigma_min}, sigma_annealing={self.cfg.sigma_annealing})); a second source is refused" if self.plain else
                             "the AR-DAE update draws its noise levels; inject them through noise={'sigma', 'eps'}"))

    def _take_noise(self, noise, sigma_buf):
        """Injected draws, validated, into the engine's own buffers (`sigma_buf`: where this engine's launches read noise['sigma']): the
        launches (and stats()) then read what a drawn step would have left there."""
        if not self.plain:
            check_tensor(noise["sigma"], "step(noise): sigma", self.dev, numel=self.N)
        check_tensor(noise["eps"], "step(noise): eps", self.dev, numel=self.eps.numel())
        if not self.plain:
            sigma_buf.copy_(noise["sigma"].reshape(-1))
        self.eps.copy_(noise["eps"].reshape(self.eps.shape))

    def _loss_grads(self, ctx, B, S):
        L.call("ardae_cdae_loss_grads", self._net._desc, self._net._flat, self.pk, self.xbar, self.sigma, self.target, ctx, B, S, self.ws, self.ws.numel(),
               self.loss, self.grads, None)

    def _draw(self, out, n, seed):
        """The step's eps draw at in-step offset 1: normals, or (a reconstruction DAE with uniform noise) uniforms in [0, 1)"""
        L.call("ardae_philox_uniform_at" if self.noise_id else "ardae_philox_normal_at", out, n, seed, 1, self.state, 0)

    def _residual_score(self, recon, x, std):
        """(recon - x) / s^2 in place of recon; s: `std`, or the device block's sigma (the coming step's) - no host synchronisation"""
        L.call("ardae_recon_score", recon, x, x.size(0), x.size(1), 0.0 if std is None else float(std), self.state if std is None else None, recon)
        return recon

    def _body(self, *front):
        self._front(*front)
        self.opt.apply(self.grads, True)      # Adam's t and bias corrections come from the device block
        L.call("ardae_cdae_pack", self._net._desc, self._net._flat, self.pk)
        self.opt.advance(RNG_STRIDE)          # for the NEXT step: Philox base += stride, t += 1

    def _run(self, drawn, *front):
        self._ladder.run(lambda: self._body(*front), eager=not drawn)
        self._count_step()

    def _count_step(self):
        self.step_count += 1
        self.opt.steps = self.step_count
        bump_versions(self._net)

    def stats(self):
        """Host copy of the last step's scalars (the only synchronising call).  A plain DAE: its loss and the finished step's sigma,
        recomputed on the host from the step count (nothing is read back for it)."""
        if not self.plain:
            return self._ar_stats()
        sigma = float(np.float32(dae_sigma(*self.sched, self.step_count - 1))) if self.step_count else float("nan")
        return dict(loss=float(self.loss), sigma=sigma)

    # ------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The network, its optimiser in torch.optim's layout, and the step count, step-state block and RNG state: everything a resumed
        run needs to continue bit-identically."""
        return {self._NET: {k: v.clone() for k, v in self._net.state_dict().items()},
                "optimizer": self.opt.state_dict(self._net),
                "engine": {"step_count": self.step_count, "rng_seed": rng.get_state()["seed"], "rng_host_offset": rng.get_state()["offset"],
                           "step_state": self.state.cpu().clone()}}

    def load_state_dict(self, sd, default_steps=0):
        """Inverse of state_dict().  Without the "engine" entry (a checkpoint assembled from torch objects) the step count is the optimiser
        state's (default_steps where that is empty: SGD) and the block is rebuilt for it: the run continues with Philox offsets it has not used."""
        self._net.load_state_dict(sd[self._NET])
        steps = self.opt.load_state_dict(self._net, sd["optimizer"], self._CHECKPOINT)
        eng = sd.get("engine")
        self.step_count = self.opt.steps = int(eng["step_count"]) if eng is not None else (steps or int(default_steps))
        if eng is not None:
            rng.manual_seed(eng["rng_seed"], eng["rng_host_offset"])
            self.state.copy_(eng["step_state"].to(self.dev))
        else:
            rebuild_step_state(self.state, self.step_count, RNG_STRIDE, lambda: self.opt.advance(RNG_STRIDE))
        if self.plain and eng is not None:
            # bytes 24..27 recomputed from t (ArdaeEngine._refresh_train_state): step the block back by one and advance it again, so that a
            # file written under another schedule resumes at THIS engine's sigma
            self.state[0] -= RNG_STRIDE
            self.state[1] -= 1
            self.opt.advance(RNG_STRIDE)
        self._ladder.reset()                    # parameters were rewritten outside of the captured step
        bump_versions(self._net)
        self.repack()


# ---------------------------------------------------------------------------------------------------------------
# Unconditional AR-DAE: the score-estimator half of notebooks/ardae_toy.ipynb / ardae_fit.ipynb
# ---------------------------------------------------------------------------------------------------------------
class ArdaeScoreEngine(_ScoreEngine):
    """One AR-DAE update of an unconditional score network (`net.MLPGradARDAE` / `net.MLPResARDAE`) as ONE captured unit:
    advance the step state, draw sigma and eps, perturb the broadcast batch, loss and gradients on B * nsigma rows, optimiser,
    re-pack.  The rules are ArdaeEngine's: `step()` is captured at its third call and replayed afterwards (replayed == eager bit for
    bit), `noise={'sigma' [B * nsigma], 'eps' [B * nsigma, d]}` runs the same launches eagerly on injected draws, batches are
    validated before any pointer reaches a kernel, in-step Philox offsets are RNG_STRIDE * step + {0 (sigma), 1 (eps)} - below
    rng.HOST_STREAM.  One stream, one linear graph; there is no data parallelism here.

    With a plain DAE (`net.MLPGradDAE` / `net.MLPResDAE`) and a `DaeConfig` the same engine runs notebooks/dae_toy.ipynb's update: no
    sigma draw - the step's one noise level is read from the device block, where `ardae_dae_state_advance` leaves the annealed value -
    so `noise` is {'eps'} alone, the in-step Philox offset RNG_STRIDE * step + 1 (eps; slot 0 stays unused), and `stats()` reports
    `loss` and `sigma`.

    With a reconstruction DAE (`net.MLPDAE`, models/dae/mlp.py) and a `DaeConfig` it is the same update with the reconstruction loss: the
    draw (normals, or uniforms in [0, 1) for noise_type='uniform') and `ardae_recon_perturb` at the block's noise level - or, `draw_form=True` (the default),
    `ardae_recon_perturb_draw`, the same bits in one launch - leave x_bar, ones and -x, on which `ardae_cdae_loss_grads` gives mse(main(x_bar), x);
    `noise={'eps'}` injects the raw draw; `score(x, std=None)` is (main(x) - x) / std^2 at the block's sigma or at `std`.

    A sampler that stays the caller's torch module takes its entropy gradient as `output.backward(engine.score(output.detach()) / B)`;
    the whole iteration of ardae_fit.ipynb on the device - generator, energy, this update - is `ArdaeFitEngine` (fit.py), which runs
    `_body(x, drawn)` inside its own captured iteration and `_count_step()` after it."""

    _NET, _AR_KINDS, _PLAIN_KINDS, _CHECKPOINT = "dae", (2, 3), (6, 7), "AR-DAE checkpoint"
    _DRIVES = ("ArdaeScoreEngine drives the unconditional networks (net.MLPGradARDAE / net.MLPResARDAE with a ScoreConfig, "
               "net.MLPGradDAE / net.MLPResDAE / net.MLPDAE with a DaeConfig)")

    RECON_DRAW_FORM_DEFAULT = True       # reconstruction DAEs: ardae_recon_perturb_draw in place of its two launches (measured: DESIGN.md section 6)

    def __init__(self, dae, cfg: ScoreConfig, batch_size, graph=True, draw_form=None):
        self._pair(dae, cfg)
        self.draw_form = self.recon and (self.RECON_DRAW_FORM_DEFAULT if draw_form is None else bool(draw_form))
        if int(cfg.nsigma) < 1 or int(batch_size) < 1:
            raise ValueError(f"nsigma and batch_size must be positive (got {cfg.nsigma}, {batch_size})")
        self.B, self.S, self.d = int(batch_size), int(cfg.nsigma), int(dae.input_dim)
        self.N = self.B * self.S
        self._allocate(dae, cfg, self.N, 1, self.d, graph)
        self.nrm = self._f(self.N)
        self._zero = torch.zeros(self.N, device=self.dev)
        self.fused_front = (not self.plain and L.debug_knob("ARDAE_FUSED_DAE_FRONT", "1") != "0"       # (the plain DAEs have no fused front end)
                            and bool(L.query("ardae_dae_perturb_fused_ok", dae._desc, self.S)))
        self._x = None

    def _check_batch(self, x, what):
        check_batch(x, what, self.dev, self.B, self.d)

    def _front(self, x, drawn):
        """Perturbation, loss and gradients of the rows of x [B, d]; drawn: the step makes its own draws (else sigma / eps hold injected ones)."""
        seed = rng.get_state()["seed"]
        if self.recon:             # sigma: the device block's in every form of the step; the loss layer reads (1, -x)
            if drawn and self.draw_form:
                L.call("ardae_recon_perturb_draw", x, self.B, self.S, self.d, self.noise_id, 0.0, self.state, seed, 1, 0, self.xbar, self.sigma,
                       self.target, self.eps)
            else:
                if drawn:
                    self._draw(self.eps, self.N * self.d, seed)
                L.call("ardae_recon_perturb", x, self.eps, self.B, self.S, self.d, self.noise_id, 0.0, self.state, self.xbar, self.sigma, self.target)
        elif self.plain:           # sigma: the device block's in every form of the step
            if drawn:
                L.call("ardae_philox_normal_at", self.eps, self.N * self.d, seed, 1, self.state, 0)
            L.call("ardae_dae_noise_perturb", x, self.eps, self.B, self.S, self.d, 0.0, self.state, self.xbar, self.sigma)
        elif drawn and self.fused_front:
            L.call("ardae_dae_perturb_loss_grads", self.dae._desc, self.dae._flat, self.pk, x, self.B, self.S, float(self.cfg.delta), seed, 0, 1,
                   self.state, 0, self.xbar, self.sigma, self.eps, self.ws, self.ws.numel(), self.loss, self.grads)
            return
        else:
            if drawn:
                L.call("ardae_philox_normal_at", self.nrm, self.N, seed, 0, self.state, 0)
                L.call("ardae_center_scale", self.nrm, self._zero, self.N, 1, 1, float(self.cfg.delta), self.sigma)     # sigma = delta * n
                L.call("ardae_philox_normal_at", self.eps, self.N * self.d, seed, 1, self.state, 0)
            L.call("ardae_dae_perturb", x, self.sigma, self.eps, self.B, self.S, self.d, self.xbar)
        self._loss_grads(None, self.N, 1)

    def step(self, x, noise=None, sigma=None):
        """One AR-DAE update on the B samples x [B, d] (each used with nsigma noise levels)."""
        self._refuse_sigma(sigma)
        self._check_batch(x, "step(x)")
        if noise is not None:
            self._take_noise(noise, self.sigma)
        elif self.use_graph and x is not self._x:
            x = self.input_buffer().copy_(x.view(self.B, self.d))      # the static batch buffer the captured launches read
        self._run(noise is None, x, noise is None)

    def input_buffer(self):
        """The static batch buffer [B, d]: a sampler that writes its batch there and passes the same tensor to step() saves the copy."""
        if self._x is None:
            self._x = self._f(self.B, self.d)
        return self._x

    def score(self, x, sigma=None, std=None):
        """glogprob(x, sigma) with the engine's weight image: x [R, d] (any R), sigma [R] / [R, 1] or None = zeros.  A reconstruction DAE:
        glogprob(x, std) = (main(x) - x) / std^2, std a number or None = the device block's sigma (the coming step's)."""
        check_tensor(x, "score(x)", self.dev, shape=(None, self.d))
        if (sigma is not None and self.recon) or (std is not None and not self.recon):
            raise ValueError("score(): a reconstruction DAE takes std= (one noise level, a number), every other network sigma= (a level per row)")
        R = x.size(0)
        s = torch.zeros(R, device=self.dev) if sigma is None else sigma.detach().to(torch.float32).reshape(-1).contiguous()
        if s.numel() != R:
            raise ValueError(f"score(sigma): {s.numel()} entries for {R} rows")
        ws = self._score_ws.get(R)
        if ws is None:
            ws = self._score_ws[R] = torch.empty(L.query("ardae_cdae_workspace_floats", self.dae._desc, R, 1, 0), device=self.dev)
        out = torch.empty(R, self.d, device=self.dev)
        L.call("ardae_cdae_score", self.dae._desc, self.dae._flat, self.pk, x.detach(), s, None, R, 1, ws, ws.numel(), out)
        return self._residual_score(out, x.detach(), std) if self.recon else out

    def _ar_stats(self):
        """The last step's loss and mean |sigma|."""
        v = torch.cat([self.loss, self.sigma.abs().mean().reshape(1)]).tolist()
        return dict(loss=v[0], sigma_abs_mean=v[1])


# ---------------------------------------------------------------------------------------------------------------
# Conditional score networks outside the VAE loop: the cDAE update of ivae_ardae.py:743-779 on the caller's samples
# ---------------------------------------------------------------------------------------------------------------
class ArdaeCondScoreEngine(_ScoreEngine):
    """One update of a CONDITIONAL score network on samples of the caller's own amortised sampler (ivae_ardae.py:752-779), as ONE captured
    unit: centre and scale the samples, perturb them, loss and gradients on B * S * nsigma rows, optimiser, re-pack, advance the step
    state.  `step(latent [B, S, z], ctx [B, c] | [B, 1, c], latent_mean=None ([B, z] | [B, 1, z]; None: zeros), noise=None)`;
    `cfg.nsigma` plays the role of --train-nstd-cdae.  The rules are ArdaeScoreEngine's: eager twice, captured at the third call, replayed
    afterwards (replayed == eager bit for bit), injected noise runs the same launches eagerly, batches are validated before any pointer
    reaches a kernel.  One stream, one linear graph; there is no data parallelism here.

    A conditional AR-DAE (`net.MLPGradCARDAE` / `net.MLPResCARDAE`) takes a `ScoreConfig`: the launches and selection rules of
    ArdaeEngine's cDAE phase behind its sampler - `ardae_cdae_perturb_loss_grads` where the shape allows, else `ardae_latent_perturb_draw`,
    else two draws and `ardae_latent_perturb_nstd` - with sigma = delta * mean_d std_S(u) * xi; `noise={'sigma': xi [N], 'eps': [N, z]}`;
    in-step Philox offsets RNG_STRIDE * step + {0 (xi), 1 (eps)}; `stats()` reports `loss` and `std_mean / std_max / std_min`.  The same
    classes with `enc_input=False` (ardae_cdae_desc.kind 16 / 17: no input encoder) run the same launches; for them the first-layer form of
    `ardae_cdae_perturb_loss_grads` is off unless `fused_first=True` asks for it (measured: DESIGN.md section 6).

    A plain conditional DAE (`net.MLPGradCDAE` / `net.MLPResCDAE`) takes a `DaeConfig`: one noise level per step, read from the device
    block where `ardae_dae_state_advance` leaves the annealed value, so the replay runs through the ramp; the launches are
    `ardae_latent_noise_perturb_draw` (`draw_form=False`, or injected eps: `ardae_philox_normal_at` and `ardae_latent_noise_perturb`, the same
    bits) and `ardae_cdae_loss_grads`; `noise={'eps'}` alone, offset RNG_STRIDE * step + 1; `stats()` reports `loss` and `sigma`.

    A reconstruction conditional DAE (`net.MLPCDAE`, models/dae/mlp.py; enc_input False or True) takes a `DaeConfig` too: the draw and
    `ardae_latent_recon_perturb` (`draw_form=True`, the default: `ardae_latent_recon_perturb_draw`, the same bits in one launch), then `ardae_cdae_loss_grads` on
    (x_bar, ones, -u) with one context per image; `score(..., std=None)` is (dae(u, ctx) - u) / std^2 at the block's sigma or at `std`.

    `score(latent, ctx, latent_mean=None)` is glogprob(std_scale (latent - mean), ctx, sigma = 0) with the engine's weight image, for any
    batch and sample size: a sampler that stays the caller's torch module takes its entropy gradient as
    `(std_scale * (latent - mean)).backward(beta * engine.score(latent.detach(), ctx, mean.detach()) / (B * S))` (ivae_ardae.py:826-834)."""

    _NET, _AR_KINDS, _PLAIN_KINDS, _CHECKPOINT = "cdae", (0, 1, 16, 17), (10, 11, 13), "cDAE checkpoint"
    _DRIVES = ("ArdaeCondScoreEngine drives the conditional networks (net.MLPGradCARDAE / net.MLPResCARDAE with a ScoreConfig, "
               "net.MLPGradCDAE / net.MLPResCDAE / net.MLPCDAE with a DaeConfig); the unconditional ones run in ArdaeScoreEngine")
    RECON_DRAW_FORM_DEFAULT = True       # reconstruction DAEs: ardae_latent_recon_perturb_draw in place of its two launches (measured: DESIGN.md section 6)
    DRAW_FORM_DEFAULT = True       # plain kinds: ardae_latent_noise_perturb_draw in place of its two launches (measured: DESIGN.md section 6)
    FUSED_FIRST_NOENC_DEFAULT = False    # kinds 16 / 17 (enc_input=False): the first energy layer inside the perturbation kernel

    def __init__(self, cdae, cfg, batch_size, sample_size, std_scale=1.0, graph=True, draw_form=None, fused_first=None):
        self._pair(cdae, cfg)
        if int(cfg.nsigma) < 1 or int(batch_size) < 1 or int(sample_size) < 1:
            raise ValueError(f"nsigma, batch_size and sample_size must be positive (got {cfg.nsigma}, {batch_size}, {sample_size})")
        if not self.plain and int(sample_size) < 2:
            raise ValueError("a conditional AR-DAE scales its noise by the unbiased std over the samples: sample_size >= 2")
        self.std_scale = float(std_scale)
        self.B, self.S, self.nstd = int(batch_size), int(sample_size), int(cfg.nsigma)
        self.z, self.c = int(cdae.input_dim), int(cdae.context_dim)
        self.N = self.B * self.S * self.nstd
        self._allocate(cdae, cfg, self.B, self.S * self.nstd, self.z, graph)
        f = self._f
        self.xi, self.std_b = f(self.N), f(self.B)
        self._latent, self._z0, self._ctx = f(self.B, self.S, self.z), torch.zeros(self.B, self.z, device=self.dev), f(self.B, self.c)
        if self.plain:
            want = (self.RECON_DRAW_FORM_DEFAULT if self.recon else self.DRAW_FORM_DEFAULT) if draw_form is None else bool(draw_form)
            # (ardae_latent_recon_perturb_draw takes every positive shape; the query is the residual kinds' kernel's)
            self.draw_form = want and (self.recon or bool(L.query("ardae_latent_noise_perturb_draw_ok", self.S, self.nstd, self.z)))
            self.fused_first = self.fused_draw = False
        else:
            self.draw_form = False
            self.fused_draw = L.debug_knob("ARDAE_FUSED_DRAW", "1") != "0" and bool(L.query("ardae_latent_perturb_draw_ok", self.S, self.nstd, self.z))
            # fused_first=None: the measured default of the network's kind (on for kinds 0 / 1); a bool asks for it, where the shape allows
            want = (int(cdae._desc.kind) < 2 or self.FUSED_FIRST_NOENC_DEFAULT) if fused_first is None else bool(fused_first)
            self.fused_first = (want and self.fused_draw and L.debug_knob("ARDAE_FUSED_A1", "1") != "0"
                                and bool(L.query("ardae_cdae_perturb_fused_ok", cdae._desc, self.S, self.nstd)))

    def _front(self, drawn):
        """Centring, perturbation, loss and gradients on the static buffers; drawn: the step makes its own draws (else xi / eps hold injected ones)."""
        seed, cfg = rng.get_state()["seed"], self.cfg
        lat, z0, B, S, nstd, z = self._latent, self._z0, self.B, self.S, self.nstd, self.z
        if self.recon:             # sigma: the device block's in every form of the step; the loss layer reads (1, -u)
            if drawn and self.draw_form:
                L.call("ardae_latent_recon_perturb_draw", lat, z0, B, S, nstd, z, self.std_scale, self.noise_id, 0.0, self.state, seed, 1, 0, self.xbar,
                       self.sigma, self.target, self.eps)
            else:
                if drawn:
                    self._draw(self.eps, self.N * z, seed)
                L.call("ardae_latent_recon_perturb", lat, z0, self.eps, B, S, nstd, z, self.std_scale, self.noise_id, 0.0, self.state, self.xbar,
                       self.sigma, self.target)
        elif self.plain:           # sigma: the device block's in every form of the step
            if drawn and self.draw_form:
                L.call("ardae_latent_noise_perturb_draw", lat, z0, B, S, nstd, z, self.std_scale, 0.0, self.state, seed, 1, 0, self.xbar, self.sigma,
                       self.eps)
            else:
                if drawn:
                    L.call("ardae_philox_normal_at", self.eps, self.N * z, seed, 1, self.state, 0)
                L.call("ardae_latent_noise_perturb", lat, z0, self.eps, B, S, nstd, z, self.std_scale, 0.0, self.state, self.xbar, self.sigma)
        elif drawn and self.fused_first:
            L.call("ardae_cdae_perturb_loss_grads", self.cdae._desc, self.cdae._flat, self.pk, lat, z0, self._ctx, B, S, self.std_scale, float(cfg.delta),
                   seed, 0, 1, self.state, 0, self.xbar, self.sigma, self.eps, self.std_b, self.ws, self.ws.numel(), self.loss, self.grads)
            return
        elif drawn and self.fused_draw:
            L.call("ardae_latent_perturb_draw", lat, z0, B, S, z, self.std_scale, float(cfg.delta), seed, 0, 1, self.state, 0, self.xbar, self.sigma,
                   self.eps, self.std_b)
        else:
            if drawn:
                L.call("ardae_philox_normal_at", self.xi, self.N, seed, 0, self.state, 0)
                L.call("ardae_philox_normal_at", self.eps, self.N * z, seed, 1, self.state, 0)
            L.call("ardae_latent_perturb_nstd", lat, z0, self.xi, self.eps, B, S, nstd, z, self.std_scale, float(cfg.delta), self.xbar, self.sigma,
                   self.std_b)
        self._loss_grads(self._ctx, B, S * nstd)

    def step(self, latent, ctx, latent_mean=None, noise=None, sigma=None):
        """One update on the samples latent [B, S, z] of the B contexts ctx (each sample used with nsigma noise draws)."""
        self._refuse_sigma(sigma)
        check_batch(latent, "step(latent)", self.dev, self.B, self.S * self.z)
        check_batch(ctx, "step(ctx)", self.dev, self.B, self.c, rows="contexts")
        if latent_mean is not None:
            check_batch(latent_mean, "step(latent_mean)", self.dev, self.B, self.z, rows="means")
        if noise is not None:
            self._take_noise(noise, self.xi)
        # the static buffers the (captured) launches read; a caller that filled input_buffers() passes the same tensors and saves the copies
        if latent is not self._latent:
            self._latent.copy_(latent.view(self.B, self.S, self.z))
        if ctx is not self._ctx:
            self._ctx.copy_(ctx.view(self.B, self.c))
        if latent_mean is None:
            self._z0.zero_()
        elif latent_mean is not self._z0:
            self._z0.copy_(latent_mean.view(self.B, self.z))
        self._run(noise is None, noise is None)

    def input_buffers(self):
        """The static (latent [B, S, z], latent_mean [B, z], ctx [B, c]) buffers: a sampler that writes there and passes the same tensors to
        step() saves the copies."""
        return self._latent, self._z0, self._ctx

    def score(self, latent, ctx, latent_mean=None, std=None):
        """glogprob(std_scale (latent - latent_mean), ctx, sigma = 0) with the engine's weight image: latent [B', S', z], ctx [B', c] | [B', 1, c],
        latent_mean [B', z] | [B', 1, z] or None = zeros -> [B', S', z].  A reconstruction DAE: glogprob(u, ctx, std) = (dae(u, ctx) - u) / std^2,
        std a number or None = the device block's sigma (the coming step's)."""
        check_tensor(latent, "score(latent)", self.dev, shape=(None, None, self.z))
        if std is not None and not self.recon:
            raise ValueError("score(std=): only a reconstruction DAE's score reads a noise level")
        Bq, Sq = latent.size(0), latent.size(1)
        check_batch(ctx, "score(ctx)", self.dev, Bq, self.c, rows="contexts")
        if latent_mean is not None:
            check_batch(latent_mean, "score(latent_mean)", self.dev, Bq, self.z, rows="means")
        bufs = self._score_ws.get((Bq, Sq))
        if bufs is None:
            bufs = self._score_ws[(Bq, Sq)] = (torch.empty(L.query("ardae_cdae_workspace_floats", self.cdae._desc, Bq, Sq, 0), device=self.dev),
                                               torch.zeros(Bq * Sq, device=self.dev), torch.zeros(Bq, self.z, device=self.dev))
        ws, sigma0, zeros = bufs
        u = torch.empty(Bq * Sq, self.z, device=self.dev)
        L.call("ardae_center_scale", latent.detach(), zeros if latent_mean is None else latent_mean.detach(), Bq, Sq, self.z, self.std_scale, u)
        out = torch.empty(Bq, Sq, self.z, device=self.dev)
        L.call("ardae_cdae_score", self.cdae._desc, self.cdae._flat, self.pk, u, None if self.plain else sigma0, ctx.detach(), Bq, Sq, ws, ws.numel(), out)
        if self.recon:
            self._residual_score(out.view(Bq * Sq, self.z), u, std)
        return out

    def _ar_stats(self):
        """The last step's loss and the per-context noise scale delta * mean_d std_S(u) - the loop's cur_mean_std*."""
        v = torch.cat([self.loss, self.std_b.mean().reshape(1), self.std_b.max().reshape(1), self.std_b.min().reshape(1)]).tolist()
        return dict(loss=v[0], std_mean=v[1], std_max=v[2], std_min=v[3])
