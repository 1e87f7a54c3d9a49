"""Posterior diagnostics of the Gaussian-posterior baselines: the compute of vae.py's `''' visualize '''` block (vae.py:497-593) and of its
`''' test visualize '''` block (vae.py:677-720) on the device.

Every `--vis-interval` steps the reference walks 20000 images in training batches, calls `model(x)` and (2-D data) `model.generate` per batch,
copies every latent and sample to the host and bins them with `np.histogram2d` at num=128; after training it does the same over 1 000 000
points at num=256.  `GaussianDiagnostics(model)` produces the same tables in large chunks (iwae.plan_chunks) without leaving the device:

    latent_histograms   z of model(x) - the encoder statistics, the draw, z = mu + exp(lv / 2) eps (the auxiliary-variable kinds: the z0 and z
                        stages of ardae_vae_aux_iwae_draw at one sample per image) - and one histogram launch per chunk; no decoder runs
    data_histograms     data | reconstruction | generation of the 2-D problems (Gaussian decoders): the reconstruction decodes the SAME z
    run                 the training block: both at 128 bins in one walk, no host synchronisation
    final_pass          the last block: both at 256 bins (latent val 4, data val 6)

Tables of up to 128 bins go through ardae_hist2d, wider ones (up to 512) through ardae_hist2d_wide (diagnostics.hist2d).  Plots, image grids
and the event file stay with the caller; these are the arrays they are drawn from.  The implicit models: diagnostics.PosteriorDiagnostics.
"""
import torch

from . import _lib as L
from . import rng
from .diagnostics import MAX_BINS_WIDE, _check_range, _val_range, cached_buffers, hist2d
from .iwae import _check, plan_chunks
from .modules import GAUSSIAN_DECODERS, GaussianVAE, _AuxGaussianVAE
from .vae import MAX_AUX

WHO = "GaussianDiagnostics"


class GaussianDiagnostics:
    """The two visualisation blocks' numbers for one Gaussian-posterior model.  Buffers are sized for the chunk length `plan` finds under
    `max_workspace_floats` (default 2^28 floats = 1 GiB), allocated at the first use and kept.

    Chunks follow GaussianIwaeEvaluator: they start on multiples of 4 images; a model with `_eval_groups` runs its encoder (and the
    auxiliary stages) on `_eval_groups[0]` images per call and cuts chunks at whole multiples of it, so every call sees the same rows under any
    budget.  The result does not depend on the budget, to the bit.

    Own draws take Philox offsets from `rng`'s host stream, one per draw and per call, in this order: the posterior draw (one offset; the
    auxiliary-variable kinds two: eps0's, then eps's - ardae_vae_aux_iwae_draw's offset0 / offset1), then, where the data histograms are
    made, the reconstruction's decoder draw, the generation's z and the generation's decoder draw - 1 (2) offsets for latent_histograms,
    4 (5) for data_histograms, run and final_pass on 2-D data.  A chunk reads its slice of each draw through `first_element` /
    `first_image`.  Injected `eps` replaces the posterior draw (and its offsets): [N, z_dim], the auxiliary-variable kinds
    [N, noise_dim + z_dim] with rows [eps0 | eps]; float32, contiguous, on the device."""

    def __init__(self, model, max_workspace_floats=1 << 28):
        if not isinstance(model, GaussianVAE):
            raise TypeError(f"{WHO} takes net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE / net.MNISTAuxVAE / net.ToyAuxVAE / "
                            "net.MNISTConvAuxVAE / net.MNISTResConvAuxVAE (the implicit models: net.PosteriorDiagnostics)")
        self.model, self.budget = model, int(max_workspace_floats)
        self.aux = isinstance(model, _AuxGaussianVAE)
        if self.aux and max(model.noise_dim, model.z_dim) > MAX_AUX:
            raise NotImplementedError(f"{WHO}: noise_dim {model.noise_dim} / z_dim {model.z_dim} > {MAX_AUX}: ardae_vae_aux_iwae_draw takes widths up "
                                      f"to {MAX_AUX}")
        self.gaussian = model._kind in GAUSSIAN_DECODERS
        self.sd = model.noise_dim if self.aux else model.z_dim      # width of the statistics ardae_vae_encode_stats returns
        self.group = (model._eval_groups or (None,))[0]             # images per encoder call (None: a chunk at once)
        self._bufs = {}

    # ---- planning ------------------------------------------------------------------------------------------------------------------
    def _ws_floats(self, c, data=False):
        d = self.model._desc
        G = min(c, self.group or c)
        need = L.query("ardae_model_workspace_floats", d, G, 1, 0)
        if self.aux:
            need = max(need, L.query("ardae_model_workspace_floats", d, G, 1, 4))
        return max(need, L.query("ardae_model_workspace_floats", d, c, 1, 2)) if data else need

    def floats_per_chunk(self, c, data=False):
        """Floats held for a chunk of c images: the workspace, the statistics, the draw, the latents (and the decoder's buffers)."""
        m = self.model
        own = 2 * self.sd + m._eps_width + m.z_dim + (1 if self.aux else 0) + ((m.z_dim + 5 * m.input_dim) if data else 0)
        return self._ws_floats(c, data) + c * own

    def plan(self, N, data=False):
        chunks = plan_chunks(N, 1, lambda c: self.floats_per_chunk(c, data), self.budget)
        G = self.group
        if G is None or len(chunks) == 1:
            return chunks
        C = (chunks[0][1] - chunks[0][0]) // G * G      # whole groups: every call starts at a multiple of its group in any plan
        if C == 0:
            raise ValueError(f"{WHO}: the budget of {self.budget} floats is below one group of {G} images ({self.floats_per_chunk(G, data)} floats)")
        return [(s, min(s + C, N)) for s in range(0, N, C)]

    # ---- the walk ------------------------------------------------------------------------------------------------------------------
    def _walk(self, x_all, latent, data, eps, keep):
        """One pass over x_all.  latent / data: (lo, hi, bins) of the latent / the data-recon-gen histograms, or None.  Every refusal comes
        before the first launch.  -> dict: latent_counts, data_counts (or None) and, with `keep`, latents, recon, gen."""
        m = self.model
        D, zd, ew, sd = m.input_dim, m.z_dim, m._eps_width, self.sd
        N = x_all.size(0) if isinstance(x_all, torch.Tensor) and x_all.dim() else 0
        _check(x_all, "x_all", (max(N, 1), 1, D), WHO)
        x = x_all.view(N, D)
        if latent is not None and zd < 2:
            raise ValueError(f"{WHO}: a 2-D histogram needs z_dim >= 2 (got {zd})")
        if data is not None and D < 2:
            raise ValueError(f"{WHO}: a 2-D histogram needs input_dim >= 2 (got {D})")
        if eps is not None:
            eps = _check(eps, "eps", (N, 1, ew), WHO).view(N, ew)
        chunks = self.plan(N, data is not None)
        m._require_gpu(x)
        with torch.no_grad():
            c0 = chunks[0][1] - chunks[0][0]
            sizes = dict(ws=self._ws_floats(c0, data is not None), mu=c0 * sd, lv=c0 * sd, eps=c0 * ew, z=c0 * zd)
            if self.aux:
                sizes["logq"] = c0
            if data is not None:
                sizes.update(zg=c0 * zd, dmu=c0 * D, dlv=c0 * D, deps=c0 * D, xs=c0 * D, xg=c0 * D)
            b = cached_buffers(self._bufs, "data" if data is not None else "latent", x.device, sizes)
            seed = rng.get_state()["seed"]
            offsets = [rng._next_offset() for _ in range(2 if self.aux else 1)] if eps is None else [0, 0]
            if data is not None:
                dec_offset, z_offset, gen_offset = rng._next_offset(), rng._next_offset(), rng._next_offset()
            d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), b["ws"]
            new = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float32)      # noqa: E731
            out = {"latent_counts": None if latent is None else torch.zeros(latent[2], latent[2], device=x.device, dtype=torch.int64),
                   "data_counts": None if data is None else torch.zeros(3, data[2], data[2], device=x.device, dtype=torch.int64)}
            if keep:
                out.update(latents=new(N, zd), recon=None if data is None else new(N, D), gen=None if data is None else new(N, D))
            for i0, i1 in chunks:
                c = i1 - i0
                xc = x[i0:i1]
                G = self.group or c
                for j in range(0, c, G):                                         # the posterior's z, `group` images per call
                    n, a = min(G, c - j), i0 + j
                    mu, lv = b["mu"][j * sd:(j + n) * sd], b["lv"][j * sd:(j + n) * sd]
                    L.call("ardae_vae_encode_stats", d, flat, packed, x[a:a + n], n, ws, ws.numel(), mu, lv)
                    if self.aux:                                                 # one sample per image: z0 from (mu0, lv0), z from q(z | z0, x)
                        L.call("ardae_vae_aux_iwae_draw", d, flat, packed, x[a:a + n], mu, lv, None if eps is None else eps[a:a + n], n, 1, seed,
                               offsets[0], offsets[1], a, ws, ws.numel(), b["z"][j * zd:(j + n) * zd], b["logq"][j:j + n], None)
                if not self.aux:                                                 # model.encode(x, eps)'s calls
                    if eps is None:
                        L.call("ardae_philox_normal_at", b["eps"], c * zd, seed, offsets[0], None, i0 * zd)
                    L.call("ardae_gaussian_sample", b["mu"], b["lv"], b["eps"] if eps is None else eps[i0:i1], c * zd, b["z"])
                if latent is not None:
                    hist2d(b["z"], c, zd, 1, 0, 0, 1, *latent, out["latent_counts"])
                if keep:
                    out["latents"][i0:i1].copy_(b["z"][:c * zd].view(c, zd))
                if data is None:
                    continue
                hist2d(xc, c, D, 1, 0, 0, 1, *data, out["data_counts"][0])
                for slot, z, offset, xs, kept in ((1, b["z"], dec_offset, b["xs"], "recon"), (2, b["zg"], gen_offset, b["xg"], "gen")):
                    if slot == 2:
                        L.call("ardae_philox_normal_at", z, c * zd, seed, z_offset, None, i0 * zd)
                    L.call("ardae_model_decode", d, flat, packed, z, c, ws, ws.numel(), b["dmu"], b["dlv"])
                    L.call("ardae_philox_normal_at", b["deps"], c * D, seed, offset, None, i0 * D)
                    L.call("ardae_gaussian_sample", b["dmu"], b["dlv"], b["deps"], c * D, xs)
                    hist2d(xs, c, D, 1, 0, 0, 1, *data, out["data_counts"][slot])
                    if keep:
                        out[kept][i0:i1].copy_(xs[:c * D].view(c, D))
        return out

    def _latent_range(self, val, bins):
        if val is None:
            val = 4.0 if self.gaussian else 6.0                                  # vae.py:540,551
        return _check_range(*_val_range(val), bins, MAX_BINS_WIDE, WHO)

    def _data_range(self, val, bins):
        if not self.gaussian:
            raise NotImplementedError(f"{WHO}: data_histograms is for the Gaussian-decoder kinds (ToyVAE, ToyAuxVAE): {type(self.model).__name__} has a "
                                      "Bernoulli decoder, and the reference histograms data, reconstruction and generation for 2-D data only")
        return _check_range(*_val_range(val), bins, MAX_BINS_WIDE, WHO)

    def _both(self):
        return self.gaussian and self.model.input_dim == 2

    # ---- the public surface --------------------------------------------------------------------------------------------------------
    def latent_histograms(self, x_all, val=None, bins=128, eps=None, return_latents=False):
        """counts [bins, bins] (int64, on the device) of np.histogram2d(z[:, 0], z[:, 1], range=[[-val, val]] * 2, bins=bins) for the z of
        model(x_all); first index the bin of latent column 0.  val: 4 for the 2-D problems, 6 for the image models (vae.py:540,551), or a
        pair (lo, hi); bins 1 .. 512.  return_latents: -> (counts, latents [N, z_dim]).  Nothing is read back."""
        out = self._walk(x_all, self._latent_range(val, bins), None, eps, return_latents)
        return (out["latent_counts"], out["latents"]) if return_latents else out["latent_counts"]

    def data_histograms(self, x_all, val=6, bins=128, eps=None, return_samples=False):
        """counts [3, bins, bins] of the 2-D problems' data-recon-gen heat maps (vae.py:532-534): slot 0 x, slot 1 the decoder sample of
        model(x) - on the z latent_histograms bins under the same `rng` state or `eps` -, slot 2 the decoder sample of model.generate
        (z ~ N(0, I)); columns 0 and 1.  return_samples: -> (counts, recon [N, D], gen [N, D], latents [N, z_dim])."""
        out = self._walk(x_all, None, self._data_range(val, bins), eps, return_samples)
        return (out["data_counts"], out["recon"], out["gen"], out["latents"]) if return_samples else out["data_counts"]

    def run(self, x_all):
        """The training block (vae.py:497-593) in one walk: {"latent_counts": [128, 128], "data_counts": [3, 128, 128] or None (data that is
        not 2-D, Bernoulli decoders)}, int64, on the device - a plot reads them when it is drawn.  No host synchronisation."""
        out = self._walk(x_all, self._latent_range(None, 128), self._data_range(6, 128) if self._both() else None, None, False)
        return {"latent_counts": out["latent_counts"], "data_counts": out["data_counts"]}

    def final_pass(self, x_all, bins=256, return_arrays=False):
        """The last block (vae.py:677-720; the reference walks 1 000 000 points at num=256): the same two histograms with latent val 4 and
        data val 6, for any kind; data_counts is None where run's is.  return_arrays adds latents [N, z_dim], recon and gen [N, D] (or None)."""
        out = self._walk(x_all, self._latent_range(4, bins), self._data_range(6, bins) if self._both() else None, None, return_arrays)
        return out if return_arrays else {"latent_counts": out["latent_counts"], "data_counts": out["data_counts"]}
