"""Posterior diagnostics on the device: the compute of the training loop's `''' visualize '''` block (ivae_ardae.py:952-1111).

Every `--vis-interval` steps the reference walks 20000 images in training batches and, per batch, calls `model.encode(x, std=s)` for
s = 0, 0.1, 0.5, 0.8, `model(x)` and `model.generate`, copies every latent to the host and bins it with `np.histogram2d`
(utils/visualization.py:193-204); once per pass it logs `log(var(forward_hidden(x, nz=64), dim=1) + 1e-10)` with its mean and median.
`PosteriorDiagnostics(model)` produces the same numbers in large chunks (iwae.plan_chunks) without leaving the device:

    latent_histograms   one scaled draw (ardae_philox_normal_scaled_at), ONE sampler call for all noise levels, one ardae_hist2d per chunk
    data_histograms     data | reconstruction | generation of the 2-D problems (Gaussian decoders), three ardae_hist2d per chunk
    logvar_qz           a sampler pass with nz rows per image + ardae_sample_logvar
    run                 the reference's pass: all three, ONE host synchronisation
    final_pass          the script's last block, `''' test visualize '''` (ivae_ardae.py:1224-1290): the two histograms at 256 bins through
                        ardae_hist2d_wide, whose table is cut into bands of x-bin rows (up to 512 bins)
The Gaussian-posterior baselines of vae.py have their own class on the same kernels: vae_diagnostics.GaussianDiagnostics.

Plots, image grids and the event file stay with the caller; these are the arrays they are drawn from.
"""
import torch

from . import _lib as L
from . import rng
from .iwae import _check, plan_chunks
from .modules import AUX_KINDS, GAUSSIAN_DECODERS

WHO = "PosteriorDiagnostics"
MAX_BINS = 128                                   # ardae_hist2d holds one bins x bins table of 32-bit counters per workgroup in LDS
STDS = (None, 0.8, 0.5, 0.1, 0.0)                # the `alllatent` panel, left to right (ivae_ardae.py:1043); None: the plain pass, std 1
TAG_MEAN, TAG_MEDIAN = "enc/logvar_qz/mean/step", "enc/logvar_qz/median/step"      # ivae_ardae.py:961-962, behind `{train_mode}/`


MAX_BINS_WIDE = 512                              # ardae_hist2d_wide cuts the table into bands of x-bin rows, one band per workgroup


def _check_range(lo, hi, bins, max_bins=MAX_BINS, who=WHO):
    lo, hi, bins = float(lo), float(hi), int(bins)
    if not 1 <= bins <= max_bins:
        why = "the kernel keeps the table in one workgroup's LDS" if max_bins == MAX_BINS else "ardae_hist2d_wide takes tables up to that width"
        raise ValueError(f"{who}: bins must be 1 .. {max_bins} (got {bins}): {why}")
    if not (hi > lo and lo > float("-inf") and hi < float("inf")):
        raise ValueError(f"{who}: the range needs finite lo < hi (got lo={lo}, hi={hi})")
    return lo, hi, bins


def _val_range(val):
    """val -> (lo, hi): a half-width, or the pair itself"""
    return val if isinstance(val, (tuple, list)) else (-float(val), float(val))


def hist2d_lds(*args):
    """ardae_hist2d: tables of up to MAX_BINS bins"""
    L.call("ardae_hist2d", *args)


def hist2d(pts, n, row_stride, nslots, slot_stride, col_x, col_y, lo, hi, bins, counts):
    """The histogram entry point for tables of up to MAX_BINS_WIDE bins: ardae_hist2d where its table fits, ardae_hist2d_wide above."""
    L.call("ardae_hist2d" if bins <= MAX_BINS else "ardae_hist2d_wide", pts, n, row_stride, nslots, slot_stride, col_x, col_y, lo, hi, bins, counts)


def cached_buffers(cache, what, device, sizes):
    """name -> float buffer of at least sizes[name] floats; kept in `cache` per `what` until a call needs a longer one."""
    b = cache.get(what)
    if b is None or b["device"] != device or any(k not in b or b[k].numel() < n for k, n in sizes.items()):
        b = dict(device=device)
        b.update({k: torch.empty(n, device=device, dtype=torch.float32) for k, n in sizes.items()})
        cache[what] = b
    return b


class PosteriorDiagnostics:
    """The visualisation block's numbers for one model.  Buffers are sized for the chunk length `plan_chunks` finds under
    `max_workspace_floats` (default 2^28 floats = 1 GiB), allocated at the first use and kept.

    Which road a kind takes in `latent_histograms` (S = len(stds) noise levels):
      stacked   mnist, toy, conv, resconv, auxmnist, auxconv, auxresconv: a sampler call with nz = S rows per image is S calls with
                nz = 1 on the same trunk (every row has its own draws and, for the aux kinds, its own z0), so ONE ardae_model_encode
                per chunk serves all levels and the per-image trunk is computed once.
      per slot  auxtoy: a call with nz rows draws sqrt(nz) z0's x sqrt(nz) z's (ivae/auxtoy.py:215,230; 5 is no square) - one nz = 1
                call per level;
                the clipped auxresconv class: its z0 keeps an UNSCALED eps0 (z0 = mu0 + (std exp(lv0 / 2) + 1) eps0), so the draw cannot be
                pre-scaled and its std = 0 pass is the random draw ardae_model_encode_hidden_raw makes for nz = 1 - one call per level,
                levels None, 1 and 0 only (the module refuses the others too).
    Both roads read the same [N, S, noise width] draw and write the same latents.

    Own noise: one Philox offset per draw and per call from `rng`'s host stream; a chunk reads its slice of each draw through
    `first_element`, so the numbers do not depend on the chunk length.  Injected noise is the UNSCALED draw, float32, contiguous, on the
    device: [N, S, noise_dim] (aux kinds: the pair ([N, S, noise_dim], [N, S, z_dim]))."""

    def __init__(self, model, max_workspace_floats=1 << 28):
        self.model, self.budget = model, int(max_workspace_floats)
        self.kind = model._kind
        self.aux = self.kind in AUX_KINDS
        self.toy = self.kind == "auxtoy"
        self.clipped = bool(getattr(model, "_clipped", False))
        self.stacked = not (self.toy or self.clipped)
        self.gaussian = self.kind in GAUSSIAN_DECODERS
        self._bufs = {}

    # ---- planning ------------------------------------------------------------------------------------------------------------------
    def _ws_floats(self, c, nz, decode_rows=0):
        d = self.model._desc
        need = L.query("ardae_model_workspace_floats", d, c, nz, 0)
        return max(need, L.query("ardae_model_workspace_floats", d, decode_rows, 1, 2)) if decode_rows else need

    def latent_floats_per_chunk(self, c, S=len(STDS)):
        """Floats held for a chunk of c images by latent_histograms: the sampler's workspace, the draw, the latents (and one slot's noise)."""
        m = self.model
        ws = self._ws_floats(c, S) if self.stacked else self._ws_floats(c, 1)
        return ws + c * S * (m._noise_width + m.z_dim) + (0 if self.stacked else c * m._noise_width)

    def data_floats_per_chunk(self, c):
        m = self.model
        return self._ws_floats(c, 1, c) + c * (m._noise_width + 2 * m.z_dim + 5 * m.input_dim)

    def _logvar_blocks(self, nz):
        """Floats per image of the sampler draws of an nz-row call, one entry per separate draw (ToyAuxIPVAE: the eps0 and the eps block)."""
        m = self.model
        return (m._q(nz) * m.noise_dim, nz * m.z_dim) if self.toy else (nz * m._noise_width,)

    def logvar_floats_per_chunk(self, c, nz=64):
        return self._ws_floats(c, nz) + c * (sum(self._logvar_blocks(nz)) + nz * self.model.z_dim)

    def plan_latent(self, N, S=len(STDS)):
        return plan_chunks(N, S, lambda c: self.latent_floats_per_chunk(c, S), self.budget)

    def plan_data(self, N):
        return plan_chunks(N, 1, self.data_floats_per_chunk, self.budget)

    def plan_logvar(self, N, nz=64):
        return plan_chunks(N, nz, lambda c: self.logvar_floats_per_chunk(c, nz), self.budget)

    def _buffers(self, what, device, sizes):
        return cached_buffers(self._bufs, what, device, sizes)

    # ---- checks (all before the first launch) --------------------------------------------------------------------------------------
    def _check_x(self, x, what):
        m = self.model
        N = x.size(0) if isinstance(x, torch.Tensor) and x.dim() else 0
        _check(x, what, (max(N, 1), 1, m.input_dim), WHO)
        return x.view(N, m.input_dim), N

    def _check_noise(self, noise, N, rows, what="noise", rows0=None):
        """-> None, one tensor [N, rows, noise_dim] or the aux pair ([N, rows0 or rows, noise_dim], [N, rows, z_dim])."""
        m = self.model
        if noise is None:
            return None
        pair = isinstance(noise, (tuple, list))
        if self.aux:
            if not pair or len(noise) != 2:
                raise ValueError(f"{WHO}: {what} of {type(m).__name__} is the pair (eps0 [N, {rows0 or rows}, noise_dim], eps [N, {rows}, z_dim])")
            return (_check(noise[0], f"{what}[0]", (N, rows0 or rows, m.noise_dim), WHO), _check(noise[1], f"{what}[1]", (N, rows, m.z_dim), WHO))
        if pair:
            raise ValueError(f"{WHO}: {what} of {type(m).__name__} is one tensor [N, {rows}, noise_dim]")
        return _check(noise, what, (N, rows, m.noise_dim), WHO)

    def _scales(self, stds):
        stds = tuple(stds)
        if not stds:
            raise ValueError(f"{WHO}: stds is empty")
        scales = [1.0 if s is None else float(s) for s in stds]
        if self.clipped and any(s not in (0.0, 1.0) for s in scales):
            raise NotImplementedError(f"{WHO}: {type(self.model).__name__} takes std None, 1 or 0 (its z0 keeps an unscaled eps0: the draw and std "
                                      "cannot be folded into one tensor)")
        return scales

    # ---- latent histograms ---------------------------------------------------------------------------------------------------------
    def latent_histograms(self, x_all, stds=STDS, val=None, bins=128, noise=None, return_latents=False):
        """counts [S, bins, bins] (int64, on the device) of np.histogram2d(z[:, 0], z[:, 1], range=[[-val, val]] * 2, bins=bins) for
        z = model.encode(x_all, std=s), one slot per entry of `stds` (None: the plain pass, forward_hidden(x)); first index the bin of
        latent column 0.  val: 4 for the 2-D problems, 6 for the image models (ivae_ardae.py:1030,1049), or a pair (lo, hi).
        return_latents: -> (counts, latents [N, S, z_dim]).  Nothing is read back."""
        return self._latent(x_all, stds, val, bins, noise, return_latents, MAX_BINS, hist2d_lds)

    def _latent(self, x_all, stds, val, bins, noise, return_latents, max_bins, hist):
        """latent_histograms with the caller's bin cap and histogram entry point"""
        m = self.model
        scales = self._scales(stds)
        S, W, zd = len(scales), m._noise_width, m.z_dim
        if val is None:
            val = 4.0 if self.gaussian else 6.0
        lo, hi, bins = _check_range(*_val_range(val), bins, max_bins)
        x, N = self._check_x(x_all, "x_all")
        if zd < 2:
            raise ValueError(f"{WHO}: a 2-D histogram needs z_dim >= 2 (got {zd})")
        noise = self._check_noise(noise, N, S)
        m._require_gpu(x)
        chunks = self.plan_latent(N, S)
        with torch.no_grad():
            c0 = chunks[0][1] - chunks[0][0]
            sizes = dict(ws=self._ws_floats(c0, S if self.stacked else 1), noise=c0 * S * W, zs=c0 * S * zd)
            if not self.stacked:
                sizes["slot"] = c0 * W
            bufs = self._buffers("latent", x.device, sizes)
            # the clipped class scales inside the sampler (std = 0: the raw call): its draw stays unscaled
            scale = torch.tensor([1.0] * S if self.clipped else scales, device=x.device, dtype=torch.float32)
            seed, offset = rng.get_state()["seed"], (rng._next_offset() if noise is None else 0)
            d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), bufs["ws"]
            counts = torch.zeros(S, bins, bins, device=x.device, dtype=torch.int64)
            latents = torch.empty(N, S, zd, device=x.device, dtype=torch.float32) if return_latents else None
            for i0, i1 in chunks:
                c = i1 - i0
                xc = x[i0:i1]
                rows = bufs["noise"][:c * S * W].view(c, S, W)
                if noise is None:
                    L.call("ardae_philox_normal_scaled_at", rows, c * S * W, seed, offset, None, i0 * S * W, W, S, scale)
                else:
                    sv = scale.view(1, S, 1)
                    if self.aux:
                        torch.mul(noise[0][i0:i1], sv, out=rows[:, :, :m.noise_dim])
                        torch.mul(noise[1][i0:i1], sv, out=rows[:, :, m.noise_dim:])
                    else:
                        torch.mul(noise[i0:i1], sv, out=rows)
                if self.stacked:
                    zs = bufs["zs"][:c * S * zd].view(c, S, zd)
                    L.call("ardae_model_encode", d, flat, packed, xc, rows, c, S, ws, ws.numel(), zs)
                    hist(zs, c, S * zd, S, zd, 0, 1, lo, hi, bins, counts)
                    if return_latents:
                        latents[i0:i1].copy_(zs)
                else:
                    zs = bufs["zs"][:S * c * zd].view(S, c, zd)                  # slot-major: every call writes its own [c, z] block
                    for s in range(S):
                        self._encode_slot(xc, rows, s, scales[s], bufs["slot"], ws, zs[s])
                    hist(zs, c, zd, S, c * zd, 0, 1, lo, hi, bins, counts)
                    if return_latents:
                        latents[i0:i1].copy_(zs.permute(1, 0, 2))
        return (counts, latents) if return_latents else counts

    def _encode_slot(self, xc, rows, s, std, slot, ws, z_out):
        """One nz = 1 sampler call on slot s of the draw `rows` [c, S, noise width] (the kinds that cannot be stacked)."""
        m = self.model
        d, flat, packed = m._desc, m._flat, m._packed_weights()
        c, nd, zd = xc.size(0), m.noise_dim, m.z_dim
        if self.clipped and std == 0.0:
            raw0 = slot[:c * nd].view(c, nd)
            raw0.copy_(rows[:, s, :nd])
            L.call("ardae_model_encode_hidden_raw", d, flat, packed, xc, raw0, c, ws, ws.numel(), z_out, None)
            return
        sn = slot[:c * m._noise_width]
        if self.toy:                                                             # [eps0 block | eps block]
            sn[:c * nd].view(c, nd).copy_(rows[:, s, :nd])
            sn[c * nd:].view(c, zd).copy_(rows[:, s, nd:])
        else:
            sn.view(c, m._noise_width).copy_(rows[:, s, :])
        L.call("ardae_model_encode", d, flat, packed, xc, sn, c, 1, ws, ws.numel(), z_out)

    # ---- data | reconstruction | generation ----------------------------------------------------------------------------------------
    def data_histograms(self, x_all, val=6, bins=128, return_samples=False):
        """counts [3, bins, bins] of the 2-D problems' data-recon-gen heat maps (ivae_ardae.py:1019-1021): slot 0 x, slot 1 the decoder
        sample of model(x) (a std = 1 latent), slot 2 the decoder sample of model.generate (z ~ N(0, I)); columns 0 and 1.  Four
        Philox offsets per call (sampler, decoder, z, decoder).  return_samples: -> (counts, recon [N, D], gen [N, D])."""
        return self._data(x_all, val, bins, return_samples, MAX_BINS, hist2d_lds)

    def _data(self, x_all, val, bins, return_samples, max_bins, hist):
        """data_histograms with the caller's bin cap and histogram entry point"""
        m = self.model
        if not self.gaussian:
            raise NotImplementedError(f"{WHO}: data_histograms is for the Gaussian-decoder kinds (toy, auxtoy): {type(m).__name__} has a Bernoulli "
                                      "decoder, and the reference histograms data, reconstruction and generation for 2-D data only")
        lo, hi, bins = _check_range(*_val_range(val), bins, max_bins)
        x, N = self._check_x(x_all, "x_all")
        D, W, zd = m.input_dim, m._noise_width, m.z_dim
        if D < 2:
            raise ValueError(f"{WHO}: a 2-D histogram needs input_dim >= 2 (got {D})")
        m._require_gpu(x)
        chunks = self.plan_data(N)
        blocks = self._logvar_blocks(1)
        with torch.no_grad():
            c0 = chunks[0][1] - chunks[0][0]
            bufs = self._buffers("data", x.device, dict(ws=self._ws_floats(c0, 1, c0), noise=c0 * W, z=c0 * zd, zg=c0 * zd, mu=c0 * D, lv=c0 * D,
                                                             eps=c0 * D, xs=c0 * D, xg=c0 * D))
            seed = rng.get_state()["seed"]
            enc_offsets = [rng._next_offset() for _ in blocks]
            dec_offset, z_offset, gen_offset = rng._next_offset(), rng._next_offset(), rng._next_offset()
            d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), bufs["ws"]
            counts = torch.zeros(3, bins, bins, device=x.device, dtype=torch.int64)
            recon = torch.empty(N, D, device=x.device, dtype=torch.float32) if return_samples else None
            gen = torch.empty(N, D, device=x.device, dtype=torch.float32) if return_samples else None
            for i0, i1 in chunks:
                c = i1 - i0
                xc = x[i0:i1]
                noise, at = bufs["noise"], 0
                for per_image, offset in zip(blocks, enc_offsets):
                    L.call("ardae_philox_normal_at", noise[at:], c * per_image, seed, offset, None, i0 * per_image)
                    at += c * per_image
                hist(xc, c, D, 1, 0, 0, 1, lo, hi, bins, counts[0])
                L.call("ardae_model_encode", d, flat, packed, xc, noise, c, 1, ws, ws.numel(), bufs["z"])
                for slot, z, offset, out, keep in ((1, bufs["z"], dec_offset, bufs["xs"], recon), (2, bufs["zg"], gen_offset, bufs["xg"], gen)):
                    if slot == 2:
                        L.call("ardae_philox_normal_at", z, c * zd, seed, z_offset, None, i0 * zd)
                    L.call("ardae_model_decode", d, flat, packed, z, c, ws, ws.numel(), bufs["mu"], bufs["lv"])
                    L.call("ardae_philox_normal_at", bufs["eps"], c * D, seed, offset, None, i0 * D)
                    L.call("ardae_gaussian_sample", bufs["mu"], bufs["lv"], bufs["eps"], c * D, out)
                    hist(out, c, D, 1, 0, 0, 1, lo, hi, bins, counts[slot])
                    if keep is not None:
                        keep[i0:i1].copy_(out[:c * D].view(c, D))
        return (counts, recon, gen) if return_samples else counts

    # ---- log var q(z) --------------------------------------------------------------------------------------------------------------
    def logvar_qz(self, x, nz=64, noise=None):
        """log(var(forward_hidden(x, nz), dim=1) + 1e-10) [N, z_dim] on the device (ivae_ardae.py:956-957; unbiased variance, centred in
        fp64).  noise: forward_hidden's draws, [N, nz, noise_dim] (aux kinds: the pair; ToyAuxIPVAE: ([N, q, noise_dim], [N, q q, z_dim]))."""
        m = self.model
        x, N = self._check_x(x, "x")
        nz = int(nz)
        if nz < 1:
            raise ValueError(f"{WHO}: nz must be >= 1 (got {nz})")
        blocks = self._logvar_blocks(nz)                                         # (ToyAuxIPVAE: raises for an nz that is no square)
        noise = self._check_noise(noise, N, nz, rows0=m._q(nz) if self.toy else None)
        zd = m.z_dim
        m._require_gpu(x)
        chunks = self.plan_logvar(N, nz)
        with torch.no_grad():
            c0 = chunks[0][1] - chunks[0][0]
            bufs = self._buffers("logvar", x.device, dict(ws=self._ws_floats(c0, nz), noise=c0 * sum(blocks), zs=c0 * nz * zd))
            seed = rng.get_state()["seed"]
            offsets = [rng._next_offset() for _ in blocks] if noise is None else None
            d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), bufs["ws"]
            out = torch.empty(N, zd, device=x.device, dtype=torch.float32)
            for i0, i1 in chunks:
                c = i1 - i0
                nb = bufs["noise"][:c * sum(blocks)]
                if noise is None:
                    at = 0
                    for per_image, offset in zip(blocks, offsets):
                        L.call("ardae_philox_normal_at", nb[at:], c * per_image, seed, offset, None, i0 * per_image)
                        at += c * per_image
                elif not self.aux:
                    nb = noise[i0:i1]                                            # the rows as they lie
                elif self.toy:
                    n0 = c * blocks[0]
                    nb[:n0].copy_(noise[0][i0:i1].reshape(-1))
                    nb[n0:].copy_(noise[1][i0:i1].reshape(-1))
                else:
                    r = nb.view(c * nz, m._noise_width)
                    r[:, :m.noise_dim].copy_(noise[0][i0:i1].reshape(c * nz, m.noise_dim))
                    r[:, m.noise_dim:].copy_(noise[1][i0:i1].reshape(c * nz, zd))
                L.call("ardae_model_encode", d, flat, packed, x[i0:i1], nb, c, nz, ws, ws.numel(), bufs["zs"])
                L.call("ardae_sample_logvar", bufs["zs"], c, nz, zd, 1e-10, out[i0:i1])
        return out

    # ---- the reference's pass ------------------------------------------------------------------------------------------------------
    def run(self, x_all, x_batch, nz=64):
        """The visualisation block: the latent (and, for 2-D data, the data-recon-gen) histograms over x_all and log var q(z) over x_batch
        (the reference takes the last training batch).  ONE host synchronisation, at the end.  -> dict: latent_counts [5, 128, 128] and
        data_counts [3, 128, 128] or None (int64, on the device - a plot reads them when it is drawn), logvar_qz (numpy [N, z_dim]),
        logvar_qz_mean, logvar_qz_median (torch.median: the lower middle value) and the two tags the reference writes."""
        self._check_x(x_batch, "x_batch")                                        # before the first launch of the pass
        latent = self.latent_histograms(x_all)
        data = self.data_histograms(x_all) if self.gaussian and self.model.input_dim == 2 else None
        lv = self.logvar_qz(x_batch, nz)
        flat = lv.reshape(-1)
        host = torch.cat([flat, flat.mean().view(1), flat.median().view(1)]).cpu()                 # the synchronisation
        mean, median = float(host[-2]), float(host[-1])
        return {"latent_counts": latent, "data_counts": data, "logvar_qz": host[:-2].view(lv.shape).numpy(), "logvar_qz_mean": mean,
                "logvar_qz_median": median, TAG_MEAN: mean, TAG_MEDIAN: median}

    # ---- the script's last block -----------------------------------------------------------------------------------------------------
    def final_pass(self, x_all, bins=256, return_arrays=False):
        """The `''' test visualize '''` block (ivae_ardae.py:1224-1290; the reference walks 1 000 000 points at num=256): the latent histograms
        of every noise level at val 4 and, for 2-D data under a Gaussian decoder, data | reconstruction | generation at val 6.  bins 1 .. 512:
        up to 128 through ardae_hist2d, above through ardae_hist2d_wide.  The clipped aux-resconv class takes its three levels, stds
        (None, 1, 0).  -> dict: latent_counts [S, bins, bins], data_counts [3, bins, bins] or None (int64, on the device; no host
        synchronisation); return_arrays adds latents [N, S, z_dim], recon and gen [N, D] (None without data_counts)."""
        stds = (None, 1, 0) if self.clipped else STDS
        with_data = self.gaussian and self.model.input_dim == 2
        latent = self._latent(x_all, stds, 4.0, bins, None, return_arrays, MAX_BINS_WIDE, hist2d)
        data = self._data(x_all, 6.0, bins, return_arrays, MAX_BINS_WIDE, hist2d) if with_data else None
        if not return_arrays:
            return {"latent_counts": latent, "data_counts": data}
        return {"latent_counts": latent[0], "data_counts": data and data[0], "latents": latent[1], "recon": data and data[1], "gen": data and data[2]}
