"""The Gaussian-posterior baselines of the reference's second trainer, vae.py, on the device: one iteration of its loop (vae.py:396-417)
as one captured unit, and its evaluate_iws (vae.py:342-377) in large chunks.

    model = net.MNISTVAE(...).cuda()          # or net.ToyVAE, net.MNISTConvVAE, net.MNISTResConvVAE, net.MNISTAuxVAE, net.ToyAuxVAE, net.MNISTConvAuxVAE, net.MNISTResConvAuxVAE
    eng = net.VaeEngine(model, net.VaeConfig(lr=1e-3, beta_init=1e-4, beta_annealing=50000), batch_size=128)
    for x in loader: eng.step(x)
    elbo, logprob = eng.evaluate_iws(x_valid, sample_size=512)
    panels = eng.diagnostics(x_vis)           # its `''' visualize '''` block: 2-D histograms of the latents (and data | recon | gen), on the device

There is one network, one stream and one linear graph per step.  There is no data parallelism here: the batch is 128 rows, the whole step
is a few dozen per-image launches, and there is nothing to shard.
"""
import contextlib
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import rng
from .engine import annealing_func
from .engine_common import RNG_STRIDE, CaptureLadder, _FlatOpt, bump_versions, check_batch, check_tensor, rebuild_step_state
from .iwae import _check, plan_chunks
from .modules import GAUSSIAN_DECODERS, GaussianVAE, _AuxGaussianVAE
from .optim import WEIGHT_AVG_KINDS, unwrap_state_dict, wrap_state_dict


@dataclass
class VaeConfig:
    """vae.py's flags (argparse defaults, vae.py:59-97)."""
    optimizer: str = "adam"        # --optimizer sgd | adam | amsgrad | rmsprop (vae.py:314-327; adam / amsgrad: the vendored Adam of utils/optim.py)
    lr: float = 1e-4               # --lr
    beta1: float = 0.5             # --beta1 (adam / amsgrad)
    momentum: float = 0.5          # --momentum (rmsprop)
    beta_init: float = 1.0         # --beta-init / --beta-fin / --beta-annealing (vae.py:397): beta rises linearly from beta_init to beta_fin over
    beta_fin: float = 1.0          # beta_annealing steps of the ZERO-based i_ep, computed on the device (ardae_train_state_advance).
    beta_annealing: int = None     # None: the constant beta_fin (annealing_func, utils/msc.py:53-55)
    weight_avg: str = "none"       # --weight-avg none | polyak | swa (vae.py:330-335), freq 1
    weight_avg_start: int = 1000   # --weight-avg-start
    weight_avg_decay: float = 0.998  # --weight-avg-decay (Polyak)
    loss_scale: float = None       # the factor of `loss = scale * loss` (vae.py:410-411); None: 1 / input_dim, the script's

    def __post_init__(self):
        if self.optimizer not in ("sgd", "adam", "amsgrad", "rmsprop"):
            raise NotImplementedError(f"unknown optimizer: {self.optimizer}")                     # vae.py:326-327
        if self.weight_avg != "none" and self.weight_avg not in WEIGHT_AVG_KINDS:
            raise NotImplementedError(f"unknown weight averaging: {self.weight_avg}")
        if int(self.weight_avg_start) < 0 or not 0.0 <= float(self.weight_avg_decay) <= 1.0:
            raise ValueError(f"weight_avg_start must be >= 0 and weight_avg_decay in [0, 1] (got {self.weight_avg_start}, {self.weight_avg_decay})")
        if self.beta_annealing is not None and (int(self.beta_annealing) != self.beta_annealing or self.beta_annealing < 1):
            raise ValueError(f"beta_annealing must be a whole number of steps >= 1, or None (got {self.beta_annealing!r})")

    def beta_schedule(self):
        """(beta_init, beta_fin, beta_annealing) of `annealing_func`, or None: a constant beta_fin."""
        if self.beta_annealing is None:
            return None
        return float(self.beta_init), float(self.beta_fin), int(self.beta_annealing)

    def beta_at(self, i_ep):
        """The KL weight of zero-based step i_ep, as vae.py:397 computes it (a Python float; the device holds numpy.float32 of it)."""
        return annealing_func(float(self.beta_init), float(self.beta_fin), None if self.beta_annealing is None else int(self.beta_annealing), int(i_ep))


MAX_Z = 64                      # ardae_vae_iwae_draw holds one sample's terms per column in LDS
MAX_AUX = 128                   # ... and ardae_vae_aux_iwae_draw's stages (noise_dim and z_dim)


class GaussianIwaeEvaluator:
    """evaluate_iws of vae.py (:342-377) for a Gaussian-posterior model.  Per chunk of images: the encoder statistics once
    (ardae_vae_encode_stats), then the ELBO rows of a forward at beta = 1 on its own draw - the KL rows from the statistics
    (ardae_vae_kld_rows), z = mu + exp(lv / 2) eps (ardae_gaussian_sample), the decoder and the reconstruction rows - and VAE.logprob -
    ardae_vae_iwae_draw, decoder, row losses, log-mean-exp.  Everything lands in [N] buffers, one row per image, which are reduced once
    at the end in an order that depends on N alone; there is no host read inside the walk.  Own draws take two Philox offsets per call
    from the host stream (the forward's, the importance samples'); a chunk reads its slice through `first_element`, so ELBO and bound do
    not depend on the chunk length, to the bit - given that a row's bits do not depend on the rows per call, which holds for the MLP families'
    layers.  Where it does not (MNISTConvVAE, MNISTResConvVAE: the library picks the kernel of every conv-as-linear by the row count), the model names fixed
    groups, `_eval_groups = (G, g)`: the encoder and the ELBO pass's decoder run on G images per call, the importance samples' decoder on g
    images per call, and chunks are whole multiples of G - so every call sees the same rows under any budget.  Injected draws: fwd_eps
    [N, z], eps [N, k, z].  There is no covariance fit and no Cholesky on this path (iwae.IwaeEvaluator is the implicit models')."""

    def __init__(self, model, sample_size, max_workspace_floats=1 << 28):
        if not isinstance(model, GaussianVAE):
            raise TypeError("GaussianIwaeEvaluator evaluates net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE / net.MNISTAuxVAE / "
                            "net.ToyAuxVAE / net.MNISTConvAuxVAE / net.MNISTResConvAuxVAE (the implicit models: net.IwaeEvaluator)")
        self.model, self.k, self.budget = model, int(sample_size), int(max_workspace_floats)
        if self.k < 1:
            raise ValueError(f"sample_size must be positive (got {sample_size})")
        self.aux = isinstance(model, _AuxGaussianVAE)      # MNISTAuxVAE / ToyAuxVAE / MNISTConvAuxVAE / MNISTResConvAuxVAE: two draws per sample, ardae_vae_aux_* in place of the head's calls
        if model.z_dim > (MAX_AUX if self.aux else MAX_Z):
            raise NotImplementedError(f"GaussianIwaeEvaluator: z_dim {model.z_dim} > {MAX_AUX if self.aux else MAX_Z}: "
                                      f"{'ardae_vae_aux_iwae_draw' if self.aux else 'ardae_vae_iwae_draw'} takes latent widths up to "
                                      f"{MAX_AUX if self.aux else MAX_Z}")
        self.gaussian = model._kind in GAUSSIAN_DECODERS
        self.sd = model.noise_dim if self.aux else model.z_dim      # width of the statistics ardae_vae_encode_stats returns
        # images per encoder / ELBO-decoder call and per importance-sample decoder call (None: a chunk at once)
        self.image_group, self.group = model._eval_groups or (None, None)
        self._bufs = None

    def _workspace_floats(self, c):
        d = self.model._desc
        G, g = min(c, self.image_group or c), min(c, self.group or c)
        aux = (L.query("ardae_model_workspace_floats", d, G, 1, 1), L.query("ardae_model_workspace_floats", d, g, self.k, 4)) if self.aux else ()
        return max(L.query("ardae_model_workspace_floats", d, G, 1, 0), L.query("ardae_model_workspace_floats", d, G, 1, 2),
                   L.query("ardae_model_workspace_floats", d, g * self.k, 1, 2), *aux)

    def _encode_stats(self, b, xc, c):
        """b["mu"], b["lv"] [c, z_dim] of the chunk xc, `self.image_group` images per encoder call"""
        m, zd = self.model, self.sd
        G = self.image_group or c
        for j in range(0, c, G):
            n = min(G, c - j)
            L.call("ardae_vae_encode_stats", m._desc, m._flat, m._packed_weights(), xc[j:j + n], n, b["ws"], b["ws"].numel(), b["mu"][j * zd:(j + n) * zd],
                   b["lv"][j * zd:(j + n) * zd])

    def _decode_rows(self, b, xc, z, c, rpi, rec, group):
        """rec [c * rpi]: the reconstruction rows of z [c * rpi, z_dim] (rpi rows per image of xc [c, input_dim]), `group` images per decoder call"""
        m, zd = self.model, self.model.z_dim
        d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), b["ws"]
        g = group or c
        for j in range(0, c, g):
            n = min(g, c - j)
            zj = z[j * rpi * zd:(j + n) * rpi * zd]
            L.call("ardae_model_decode", d, flat, packed, zj, n * rpi, ws, ws.numel(), b["out0"], b["out1"])
            L.call("ardae_model_loss_rows", d, b["out0"], b["out1"], xc[j:j + n], zj, n * rpi, rpi, rec[j * rpi:(j + n) * rpi], b["pri"][j * rpi:(j + n) * rpi])

    def floats_per_chunk(self, c):
        m, k = self.model, self.k
        own = 2 * m.z_dim + 2 * self.sd + k * m.z_dim + 3 * k + (2 if self.gaussian else 1) * k * m.input_dim
        return self._workspace_floats(c) + c * own

    def plan(self, N):
        chunks = plan_chunks(N, self.k, self.floats_per_chunk, self.budget)
        if self.aux and self.image_group is None and len(chunks) > 1:
            # own draws are keyed by a chunk's first image, and a Philox counter holds 4 normals: chunks start at multiples of 4 images
            C = (chunks[0][1] - chunks[0][0]) // 4 * 4
            if C == 0:
                raise ValueError(f"GaussianIwaeEvaluator: the budget of {self.budget} floats is below 4 images ({self.floats_per_chunk(4)} floats)")
            return [(s, min(s + C, N)) for s in range(0, N, C)]
        G = self.image_group
        if G is None or len(chunks) == 1:
            return chunks
        C = (chunks[0][1] - chunks[0][0]) // G * G      # whole groups: every call starts at a multiple of its group in any plan
        if C == 0:
            raise ValueError(f"GaussianIwaeEvaluator: the budget of {self.budget} floats is below one group of {G} images "
                             f"({self.floats_per_chunk(G)} floats)")
        return [(s, min(s + C, N)) for s in range(0, N, C)]

    def _buffers(self, c, device):
        if self._bufs is None or self._bufs["c"] < c or self._bufs["ws"].device != device:
            m, k = self.model, self.k
            new = lambda *shape: torch.empty(*shape, device=device, dtype=torch.float32)      # noqa: E731
            self._bufs = dict(c=c, ws=new(self._workspace_floats(c)), feps=new(c * m.z_dim), fz=new(c * m.z_dim), mu=new(c * self.sd), lv=new(c * self.sd),
                              z=new(c * k * m.z_dim), logq=new(c * k), rec=new(c * k), pri=new(c * k), out0=new(c * k * m.input_dim),
                              out1=new(c * k * m.input_dim) if self.gaussian else None)
        return self._bufs

    def evaluate_rows(self, x_all, eps=None, fwd_eps=None):
        """-> (recon [N], kld [N], IWAE bound [N]) of every image, on the device; nothing is read back."""
        m, k, zd = self.model, self.k, self.model.z_dim
        N = x_all.size(0) if isinstance(x_all, torch.Tensor) and x_all.dim() else 0
        who = "GaussianIwaeEvaluator"
        _check(x_all, "x_all", (max(N, 1), 1, m.input_dim), who)
        m._require_gpu(x_all)
        if eps is not None:
            eps = _check(eps, "eps", (N, k, m._eps_width), who)
        if fwd_eps is not None:
            fwd_eps = _check(fwd_eps, "fwd_eps", (N, 1, m._eps_width), who)
        if self.aux:
            return self._evaluate_rows_aux(x_all.view(N, m.input_dim), N, eps, fwd_eps)
        x = x_all.view(N, m.input_dim)
        chunks = self.plan(N)
        with torch.no_grad():
            b = self._buffers(chunks[0][1] - chunks[0][0], x.device)
            seed = rng.get_state()["seed"]
            fwd_offset = rng._next_offset() if fwd_eps is None else 0
            iw_offset = rng._next_offset() if eps is None else 0
            d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), b["ws"]
            recon, kld, out = (torch.empty(N, device=x.device, dtype=torch.float32) for _ in range(3))
            for i0, i1 in chunks:
                c = i1 - i0
                xc = x[i0:i1]
                self._encode_stats(b, xc, c)
                # the forward at beta = 1 (vae.py:360), row by row
                if fwd_eps is None:
                    L.call("ardae_philox_normal_at", b["feps"], c * zd, seed, fwd_offset, None, i0 * zd)
                    fe = b["feps"]
                else:
                    fe = fwd_eps.view(N, zd)[i0:i1]
                L.call("ardae_vae_kld_rows", b["mu"], b["lv"], c, zd, kld[i0:i1])
                L.call("ardae_gaussian_sample", b["mu"], b["lv"], fe, c * zd, b["fz"])
                self._decode_rows(b, xc, b["fz"], c, 1, recon[i0:i1], self.image_group)
                # model.logprob (vae.py:363)
                L.call("ardae_vae_iwae_draw", b["mu"], b["lv"], None if eps is None else eps[i0:i1], c, k, zd, seed, iw_offset, i0 * k * zd, b["z"],
                       b["logq"], None)
                self._decode_rows(b, xc, b["z"], c, k, b["rec"], self.group)
                L.call("ardae_iwae_reduce", b["rec"], b["pri"], b["logq"], c, k, out[i0:i1])
        return recon, kld, out

    def _evaluate_rows_aux(self, x, N, eps, fwd_eps):
        """evaluate_rows for MNISTAuxVAE / ToyAuxVAE: per chunk the statistics of q(z0 | x), the ELBO rows of a forward at beta = 1
        (ardae_vae_aux_elbo_rows: recon and kld + aux_kld), then VAE.logprob - ardae_vae_aux_iwae_draw, decoder, row losses, log-mean-exp.  Own draws
        take four Philox offsets per call (two per pass: z0's and z's), each keyed by the chunk's first image.  Injected: fwd_eps
        [N, noise_dim + z_dim], eps [N, k, noise_dim + z_dim]."""
        m, k, w = self.model, self.k, self.model._eps_width
        chunks = self.plan(N)
        with torch.no_grad():
            b = self._buffers(chunks[0][1] - chunks[0][0], x.device)
            seed = rng.get_state()["seed"]
            f0, f1 = (rng._next_offset(), rng._next_offset()) if fwd_eps is None else (0, 0)
            o0, o1 = (rng._next_offset(), rng._next_offset()) if eps is None else (0, 0)
            d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), b["ws"]
            recon, kld, out = (torch.empty(N, device=x.device, dtype=torch.float32) for _ in range(3))
            for i0, i1 in chunks:
                c = i1 - i0
                xc = x[i0:i1]
                self._encode_stats(b, xc, c)
                # (a model with fixed groups: the ELBO pass on image_group images per call, the three stages on group images per call - whole groups
                # start at multiples of 4 images, as the draws' keying asks)
                G, g = self.image_group or c, self.group or c
                for j in range(0, c, G):
                    n, a = min(G, c - j), i0 + j
                    L.call("ardae_vae_aux_elbo_rows", d, flat, packed, x[a:a + n], None if fwd_eps is None else fwd_eps.view(N, w)[a:a + n], n, seed, f0, f1,
                           a, ws, ws.numel(), recon[a:a + n], kld[a:a + n])
                for j in range(0, c, g):
                    n, a = min(g, c - j), i0 + j
                    L.call("ardae_vae_aux_iwae_draw", d, flat, packed, x[a:a + n], b["mu"][j * self.sd:(j + n) * self.sd], b["lv"][j * self.sd:(j + n) * self.sd],
                           None if eps is None else eps[a:a + n], n, k, seed, o0, o1, a, ws, ws.numel(), b["z"][j * k * m.z_dim:(j + n) * k * m.z_dim],
                           b["logq"][j * k:(j + n) * k], None)
                self._decode_rows(b, xc, b["z"], c, k, b["rec"], self.group)
                L.call("ardae_iwae_reduce", b["rec"], b["pri"], b["logq"], c, k, out[i0:i1])
        return recon, kld, out

    def evaluate(self, x_all, eps=None, fwd_eps=None):
        """-> (elbo, logprob): the means over x_all of -(recon + kld) at beta = 1 and of the IWAE bound (evaluate_iws' `total_elbo / num_data`,
        `total_logprob / num_data`), each one reduction of an [N] buffer in double; one host synchronisation."""
        recon, kld, rows = self.evaluate_rows(x_all, eps, fwd_eps)
        elbo, logprob = torch.stack([-(recon.double() + kld.double()).mean(), rows.double().mean()]).tolist()
        return elbo, logprob


class VaeEngine:
    """One iteration of vae.py's train loop (:396-417) as ONE captured unit on one stream: forward with the posterior draw made inside the
    head kernel, backward (loss scaled by `cfg.loss_scale`), optimiser, re-pack, optional weight average, advance of the device block.  The
    rules are ArdaeScoreEngine's: `step()` is captured at its third call and replayed afterwards (replayed == eager bit for bit), `eps`
    [B, z] runs the same launches eagerly on an injected draw, batches are validated before any pointer reaches a kernel, the in-step
    Philox offset is RNG_STRIDE * step + 0 - below rng.HOST_STREAM.  With a beta schedule the KL weight of the coming step lives in the
    device block (`ardae_train_state_advance`, on the zero-based i_ep like vae.py:394-397) and both passes read it there, so the replay
    runs through the ramp.  There is no data parallelism: the batch is 128 rows and there is nothing to shard."""

    RNG_STRIDE = RNG_STRIDE

    def __init__(self, model, cfg: VaeConfig, batch_size, graph=True):
        if not isinstance(model, GaussianVAE):
            raise TypeError("VaeEngine drives the Gaussian-posterior baselines (net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE / "
                            "net.MNISTAuxVAE / net.ToyAuxVAE / net.MNISTConvAuxVAE / net.MNISTResConvAuxVAE); the implicit models take net.ArdaeEngine")
        if not isinstance(cfg, VaeConfig):
            raise TypeError(f"VaeEngine takes a VaeConfig, not a {type(cfg).__name__}")
        model._require_gpu()
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be positive (got {batch_size})")
        self.model, self.cfg, self.B = model, cfg, int(batch_size)
        self.dev = model._flat.device
        self.D, self.zd = model.input_dim, model.z_dim
        self.loss_scale = 1.0 / float(self.D) if cfg.loss_scale is None else float(cfg.loss_scale)
        f = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
        self.ws = f(L.query("ardae_model_workspace_floats", model._desc, self.B, 1, 1))
        self.ew = model._eps_width                              # floats per image of the step's draw (z_dim; the auxiliary-variable models: noise_dim + z_dim)
        self.z, self.eps, self.losses = f(self.B, self.zd), f(self.B, self.ew), f(3)
        self.grads = torch.zeros_like(model._flat)
        self.state = torch.zeros(4, dtype=torch.int64, device=self.dev)
        self._state_f32 = self.state.view(torch.float32)       # float 6: the block's beta
        self._beta_done = f(1)                                  # the beta of the last finished step, copied out before the block advances
        self.sched = cfg.beta_schedule()
        train = None if self.sched is None else self.sched + (1.0, 1)      # (no entropy seed here: std_scale 1, one seed row)
        self.opt = _FlatOpt(cfg.optimizer, model._flat, model._flat.numel(), cfg.lr, cfg.beta1, cfg.momentum, state=self.state, train=train)
        self.wavg = None if cfg.weight_avg == "none" else cfg.weight_avg
        self.avg = torch.zeros_like(model._flat) if self.wavg else None
        self._avg_origin = int(cfg.weight_avg_start) + 1
        self._avg_swap = None
        self._iwae = None
        self._diag = None
        self._ladder = CaptureLadder(self.dev, graph)
        self._x = None
        self.step_count = 0
        self.opt.advance(self.RNG_STRIDE)      # the block always describes the COMING step (t = 1, beta of i_ep = 0)
        self.repack()

    def repack(self):
        self.model._packed = None
        self.pk = self.model._packed_weights()

    _graph = property(lambda self: self._ladder.graph)
    use_graph = property(lambda self: self._ladder.on, lambda self, on: setattr(self._ladder, "on", bool(on)))

    def _check_batch(self, x, what):
        check_batch(x, what, self.dev, self.B, self.D, "images")

    def _body(self, x, eps):
        m, d, seed = self.model, self.model._desc, rng.get_state()["seed"]
        if self.sched is None:
            beta = float(self.cfg.beta_fin)
            L.call("ardae_vae_forward", d, m._flat, self.pk, x, eps, self.B, beta, self.loss_scale, seed, 0, self.state, self.ws, self.ws.numel(),
                   self.z, self.eps, self.losses)
            L.call("ardae_vae_backward", d, m._flat, self.pk, x, self.B, beta, self.loss_scale, self.ws, self.ws.numel(), self.grads, 0.0)
        else:
            L.call("ardae_vae_forward_dev", d, m._flat, self.pk, x, eps, self.B, self.state, self.loss_scale, seed, 0, self.state, self.ws,
                   self.ws.numel(), self.z, self.eps, self.losses)
            L.call("ardae_vae_backward_dev", d, m._flat, self.pk, x, self.B, self.state, self.loss_scale, self.ws, self.ws.numel(), self.grads, 0.0)
            torch.mul(self._state_f32[6:7], 1.0, out=self._beta_done)      # (an element-wise kernel, not a copy node: see elementwise.h)
        self.opt.apply(self.grads, True)       # Adam's t and bias corrections come from the device block
        L.call("ardae_model_pack", d, m._flat, self.pk)
        if self.avg is not None:               # t from the block (not yet advanced): a replayed graph averages at the right steps
            L.call("ardae_weight_avg", self.avg, m._flat, self.avg.numel(), WEIGHT_AVG_KINDS[self.wavg], float(self.cfg.weight_avg_decay),
                   self._avg_origin, self.state, 0)
        self.opt.advance(self.RNG_STRIDE)      # for the NEXT step: Philox base += stride, t += 1, beta of the next i_ep

    def step(self, x, eps=None):
        """One update on the B images x [B, ...]; eps [B, z_dim] injects the posterior draw (parity tests; MNISTAuxVAE / ToyAuxVAE:
        [B, noise_dim + z_dim], rows [eps0 | eps])."""
        self._require_trained("step()")
        self._check_batch(x, "step(x)")
        if eps is not None:
            check_tensor(eps, "step(eps)", self.dev, numel=self.B * self.ew)
        if self.use_graph and eps is None and x is not self._x:
            x = self.input_buffer().copy_(x.reshape(self.B, self.D))       # the static batch buffer the captured launches read
        else:
            x = x.reshape(self.B, self.D)
        self._ladder.run(lambda: self._body(x, eps), eager=eps is not None)
        self.step_count += 1
        self.opt.steps = self.step_count
        bump_versions(self.model)

    def input_buffer(self):
        """The static batch buffer [B, input_dim]: a loader that writes its batch there and passes the same tensor to step() saves the copy."""
        if self._x is None:
            self._x = torch.empty(self.B, self.D, device=self.dev, dtype=torch.float32)
        return self._x

    def beta_of_step(self, step):
        """numpy.float32 of vae.py:397's beta for the `step`-th update (1-based), as the device block holds it."""
        return float(np.float32(self.cfg.beta_at(step - 1)))

    def stats(self):
        """Host copy of the last step's scalars (the only synchronising call): loss (unscaled, as VAE.forward returns it), recon, kld,
        elbo = -(recon + kld), and the beta the step ran with - read from the device where a schedule is set."""
        if self.sched is None:
            v, beta = self.losses.tolist(), float(np.float32(self.cfg.beta_fin))
        else:
            *v, beta = torch.cat([self.losses, self._beta_done]).tolist()
        return dict(loss=v[0], recon=v[1], kld=v[2], elbo=-(v[1] + v[2]), beta=beta)

    # ------------------------------------------------------------------------------------------------------------
    def _n_avg(self):
        return max(0, self.step_count - self._avg_origin + 1)

    def state_dict(self):
        """The network, its optimiser in torch.optim's layout (with --weight-avg: in the wrapper layout of optim.py, averaged weights
        included), the step count, the device block and the RNG state: a resumed run continues bit-identically."""
        self._require_trained("state_dict()")
        opt = self.opt.state_dict(self.model)
        if self.avg is not None:
            n_avg = self._n_avg()
            opt["param_groups"][0].update(n_avg=n_avg, step_counter=self.step_count)
            opt = wrap_state_dict(opt, self.wavg, dict(enumerate(v.clone() for v in self.model.param_views(self.avg))) if n_avg else {})
        return {"state_dict": {k: v.clone() for k, v in self.model.state_dict().items()}, "optimizer": opt,
                "engine": {"step_count": self.step_count, "rng_seed": rng.get_state()["seed"], "rng_host_offset": rng.get_state()["offset"],
                           "step_state": self.state.cpu().clone()}}

    def load_state_dict(self, sd, default_steps=0):
        """Inverse of state_dict(); without the "engine" entry (a file written by the reference loop or the module path) the block is rebuilt
        for the optimiser's step count.  Whatever the file's block says of beta, this engine's schedule at the block's t holds."""
        self._require_trained("load_state_dict()")
        inner, w_kind, w_bufs = unwrap_state_dict(sd["optimizer"])
        if self.avg is not None and w_kind is not None and w_kind != self.wavg:
            raise ValueError(f"checkpoint: holds a {w_kind!r} average, but this engine was built with weight_avg={self.wavg!r}")
        self.model.load_state_dict(sd["state_dict"])
        steps = self.opt.load_state_dict(self.model, inner, "VAE checkpoint")
        eng = sd.get("engine")
        self.step_count = self.opt.steps = int(eng["step_count"]) if eng is not None else (steps or int(default_steps))
        if eng is not None:
            rng.manual_seed(eng["rng_seed"], eng["rng_host_offset"])
            self.state.copy_(eng["step_state"].to(self.dev))
            if self.sched is not None:          # bytes 24..27 recomputed from t: step the block back by one and advance it again
                self.state[0] -= self.RNG_STRIDE
                self.state[1] -= 1
                self.opt.advance(self.RNG_STRIDE)
        else:
            rebuild_step_state(self.state, self.step_count, self.RNG_STRIDE, lambda: self.opt.advance(self.RNG_STRIDE))
        if self.avg is not None:
            n_avg = int((inner.get("param_groups") or [{}])[0].get("n_avg", 0)) if w_kind is not None else 0
            if n_avg > 0:
                with torch.no_grad():
                    for i, v in enumerate(self.model.param_views(self.avg)):
                        v.copy_(w_bufs[i])
                self._avg_origin = self.step_count + 1 - n_avg
            else:
                self._avg_origin = max(int(self.cfg.weight_avg_start), self.step_count) + 1
        self._ladder.reset()                    # parameters were rewritten outside of the captured step
        bump_versions(self.model)
        self.repack()

    # ---- weight averaging (vae.py:330-335,344-345,375-376), as on ArdaeEngine ------------------------------------------------------
    def _require_trained(self, what):
        if self._avg_swap is not None:
            raise RuntimeError(f"VaeEngine.{what} while the averaged weights are in: call use_trained() first")

    def _swap_average(self):
        with torch.no_grad():
            tmp = self.model._flat.clone()
            self.model._flat.copy_(self.avg)
            self.avg.copy_(tmp)
        bump_versions(self.model)
        self.model.mark_dirty()
        L.call("ardae_model_pack", self.model._desc, self.model._flat, self.pk)

    def use_averaged(self):
        """optimizer.use_buf() (vae.py:344-345): the averaged weights into model._flat, in place; before the first averaging step the raw
        weights stay.  step() and the checkpoints are refused until use_trained()."""
        if self.avg is None:
            raise RuntimeError("use_averaged(): this engine was built with weight_avg='none'")
        if self._avg_swap is not None:
            return
        self._avg_swap = self._n_avg() > 0
        if self._avg_swap:
            self._swap_average()

    def use_trained(self):
        """optimizer.use_sgd() (vae.py:375-376): the trained weights back, bit for bit."""
        if self._avg_swap is None:
            return
        if self._avg_swap:
            self._swap_average()
        self._avg_swap = None

    @contextlib.contextmanager
    def averaged_weights(self):
        """with engine.averaged_weights(): ll = model.logprob(x) - use_averaged() ... use_trained()."""
        self.use_averaged()
        try:
            yield self.model
        finally:
            self.use_trained()

    def averaged_params(self):
        """The averaged weights as a flat tensor in named_parameters() order (None before the first averaging step)."""
        if self.avg is None or self._n_avg() == 0:
            return None
        return self.model._flat if self._avg_swap else self.avg

    def evaluate_iws(self, x_all, sample_size, eps=None, fwd_eps=None, max_workspace_floats=None):
        """evaluate_iws (vae.py:342-377) -> (elbo, logprob): the means over x_all [N, ...] of -(recon + kld) of a forward at beta = 1 and of
        the IWAE-`sample_size` bound under the analytic posterior, in chunks planned by iwae.plan_chunks, one host synchronisation
        (GaussianIwaeEvaluator).  With weight averaging it evaluates the averaged weights and puts the trained ones back bit for bit."""
        key = (int(sample_size), max_workspace_floats)
        if self._iwae is None or self._iwae[0] != key:
            kw = {} if max_workspace_floats is None else {"max_workspace_floats": max_workspace_floats}
            self._iwae = (key, GaussianIwaeEvaluator(self.model, sample_size, **kw))
        ev = self._iwae[1]
        if self.wavg is None or self._avg_swap is not None:
            return ev.evaluate(x_all, eps, fwd_eps)
        with self.averaged_weights():
            return ev.evaluate(x_all, eps, fwd_eps)

    def diagnostics(self, x_all):
        """The visualisation block (vae.py:497-593) on the device: vae_diagnostics.GaussianDiagnostics.run on the engine's model with the LIVE
        weights, as the reference's block reads them (the averaged weights are swapped in for evaluate_iws only; while they are in, this is
        refused like step()).  It consumes host-stream Philox offsets and nothing of the step's state, graph or in-step Philox base."""
        self._require_trained("diagnostics()")
        if self._diag is None:
            from .vae_diagnostics import GaussianDiagnostics      # (that module reads this one's width limits)
            self._diag = GaussianDiagnostics(self.model)
        return self._diag.run(x_all)
