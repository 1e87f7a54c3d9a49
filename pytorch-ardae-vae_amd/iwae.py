"""IWAE evaluation of a whole set on the device (evaluate_iws, ivae_ardae.py:644-673, around logprob_w_cov_gaussian_posterior,
ivae/mnist.py:378-437).

`IwaeEvaluator(model, k).evaluate(x_all)` walks x_all [N, ...] in large chunks.  Per chunk: the sampler (ardae_model_encode), the fused
proposal kernel (ardae_iwae_proposal: mean, covariance, Cholesky factor, proposal samples and their log-density in one launch), the
decoder (ardae_model_decode), the row losses (ardae_model_loss_rows) and the log-mean-exp (ardae_iwae_reduce) into one [N] buffer -
five launches plus the model's own, no host read.  `evaluate` synchronises once, at the end, for the finiteness check and the mean.
`model.logprob` is the drop-in surface and stays what it is; this is the path an evaluation loop should take.
"""
import torch

from . import _lib as L
from . import rng
from .modules import AUX_KINDS, GAUSSIAN_DECODERS

MAX_Z = 64                      # the proposal kernel holds one z x z matrix per workgroup in LDS
MAX_ROWS = 2 ** 31 - 1          # the C ABI counts rows in `int`
NOT_PD = "logprob: a sample covariance is not positive definite (torch.distributions would raise here too)"


def plan_chunks(N, rows_per_image, floats_per_image, budget):
    """-> [(start, stop), ...] covering [0, N) once, in order.  Every start is a multiple of 4 (a chunk's slice of a Philox draw starts
    on a counter: 4 normals), every chunk is as long as the others (the last may be shorter), holds at most 2^31 - 1 rows
    (`rows_per_image` each) and needs at most `budget` floats.  `floats_per_image`: floats per image (a number), or a function
    `images -> floats` for needs that are not proportional (workspace queries).  A budget below a chunk of 4 images raises."""
    N, rows_per_image = int(N), int(rows_per_image)
    if N <= 0 or rows_per_image <= 0:
        raise ValueError(f"plan_chunks: need N > 0 and rows_per_image > 0 (got {N}, {rows_per_image})")
    need = floats_per_image if callable(floats_per_image) else (lambda c: c * floats_per_image)
    if need(4) > budget or 4 * rows_per_image > MAX_ROWS:
        raise ValueError(f"plan_chunks: a chunk of 4 images needs {need(4)} floats and {4 * rows_per_image} rows; the budget is {budget} floats "
                         f"and {MAX_ROWS} rows")
    lo, hi = 1, (N + 3) // 4                      # chunk length in units of 4 images: the largest that fits, by bisection
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if need(4 * mid) <= budget and 4 * mid * rows_per_image <= MAX_ROWS:
            lo = mid
        else:
            hi = mid - 1
    nchunks = -(-N // (4 * lo))
    C = 4 * -(-N // (4 * nchunks))                # equal chunks: no short tail behind long ones
    return [(s, min(s + C, N)) for s in range(0, N, C)]


def _check(t, what, shape, who="IwaeEvaluator"):
    """float32, contiguous, on the device, `shape` (leading dimension and element count) - in this order, before anything is launched."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{who}: {what}: expected a float32 tensor on the GPU, got {getattr(t, 'dtype', type(t))}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be contiguous (chunks are passed as slices of it)")
    if not t.is_cuda:
        raise TypeError(f"{who}: {what}: expected a float32 tensor on the GPU, got {t.dtype} on {t.device}")
    if t.dim() < 1 or t.size(0) != shape[0] or t.numel() != shape[0] * shape[1] * shape[2]:
        raise ValueError(f"{who}: {what} must be {list(shape)}, got {list(t.shape)}")
    return t


class IwaeEvaluator:
    """evaluate_iws for one model and sample size.  Buffers are sized for the chunk length `plan_chunks` finds under `max_workspace_floats`
    (default 2^28 floats = 1 GiB), allocated at the first use and kept.

    Own noise: one Philox offset per draw and per call from `rng`'s host stream (the encoder draw, the proposal draw; ToyAuxIPVAE's
    two-block layout takes one offset per block, so three in all); a chunk reads its slice of each draw through `first_element`, so the
    numbers, and with them the result, do not depend on the chunk length - for every model kind, ToyAuxIPVAE included.
    Injected noise has logprob's shapes: enc_noise [N, k, noise_dim] (aux models: the pair ([N, k, noise_dim], [N, k, z]); ToyAuxIPVAE:
    ([N, k, noise_dim], [N, k k, z])), prop_noise [N, k, z]; float32, on the device, contiguous."""

    def __init__(self, model, sample_size, max_workspace_floats=1 << 28):
        self.model, self.k, self.budget = model, int(sample_size), int(max_workspace_floats)
        if model.z_dim > MAX_Z:
            raise NotImplementedError(f"IwaeEvaluator: z_dim {model.z_dim} > {MAX_Z}: the proposal kernel holds one z x z matrix per workgroup "
                                      "(model.logprob takes larger latent spaces)")
        if self.k < 2 * model.z_dim:
            raise AssertionError(f"sample_size >= 2 * z_dim (got {self.k}, z_dim {model.z_dim})")          # ivae/mnist.py:382
        self.toy = model._kind == "auxtoy"
        self.ke = self.k * self.k if self.toy else self.k            # ToyAuxIPVAE: k z0's x k z's (ivae/auxtoy.py:313)
        self.jitter = 1e-5 if model._kind in AUX_KINDS else 0.0      # ivae/auxmnist.py:321, ivae/auxconv.py, ivae/auxresconv.py:299
        self.gaussian = model._kind in GAUSSIAN_DECODERS
        # floats of a chunk's sampler noise per image, as the blocks of separate draws
        self.noise_blocks = (self.k * model.noise_dim, self.ke * model.z_dim) if self.toy else (self.k * model._noise_width,)
        self._bufs = None

    # ---- planning ------------------------------------------------------------------------------------------------------------------
    def _workspace_floats(self, c):
        d = self.model._desc
        return max(L.query("ardae_model_workspace_floats", d, c, self.ke, 0), L.query("ardae_model_workspace_floats", d, c * self.k, 1, 2))

    def floats_per_chunk(self, c):
        """Floats the evaluator holds for a chunk of c images: the sampler's / decoder's workspace (one buffer, used in turn) and its own."""
        m, k = self.model, self.k
        own = sum(self.noise_blocks) + self.ke * m.z_dim + k * m.z_dim + 3 * k + (2 if self.gaussian else 1) * k * m.input_dim
        return self._workspace_floats(c) + c * own

    def plan(self, N):
        return plan_chunks(N, self.ke, self.floats_per_chunk, self.budget)

    def _buffers(self, c, device):
        if self._bufs is None or self._bufs["c"] < c or self._bufs["ws"].device != device:
            m, k = self.model, self.k
            new = lambda *shape: torch.empty(*shape, device=device, dtype=torch.float32)      # noqa: E731
            self._bufs = dict(c=c, ws=new(self._workspace_floats(c)), noise=new(c * sum(self.noise_blocks)), zs=new(c * self.ke * m.z_dim),
                              newz=new(c * k * m.z_dim), logq=new(c * k), rec=new(c * k), pri=new(c * k), out0=new(c * k * m.input_dim),
                              out1=new(c * k * m.input_dim) if self.gaussian else None)
        return self._bufs

    # ---- noise ---------------------------------------------------------------------------------------------------------------------
    def _check_noise(self, N, enc_noise, prop_noise):
        m, k = self.model, self.k
        if enc_noise is not None:
            pair = isinstance(enc_noise, (tuple, list))
            if m._kind in AUX_KINDS:
                if not pair or len(enc_noise) != 2:
                    raise ValueError(f"IwaeEvaluator: enc_noise of {type(m).__name__} is the pair (eps0 [N, k, noise_dim], eps [N, {'k k' if self.toy else 'k'}, z_dim])")
                enc_noise = (_check(enc_noise[0], "enc_noise[0]", (N, k, m.noise_dim)), _check(enc_noise[1], "enc_noise[1]", (N, self.ke, m.z_dim)))
            else:
                if pair:
                    raise ValueError(f"IwaeEvaluator: enc_noise of {type(m).__name__} is one tensor [N, k, noise_dim]")
                enc_noise = _check(enc_noise, "enc_noise", (N, k, m.noise_dim))
        if prop_noise is not None:
            prop_noise = _check(prop_noise, "prop_noise", (N, k, m.z_dim))
        return enc_noise, prop_noise

    def _chunk_noise(self, bufs, i0, c, enc_noise, seed, offsets):
        """The sampler noise of images [i0, i0 + c) as ardae_model_encode reads it."""
        m, k = self.model, self.k
        if enc_noise is not None and not isinstance(enc_noise, tuple):
            return enc_noise[i0:i0 + c]                                         # [c, k, noise_dim]: the rows as they lie
        noise = bufs["noise"][:c * sum(self.noise_blocks)]
        if enc_noise is None:
            at = 0
            for per_image, offset in zip(self.noise_blocks, offsets):
                L.call("ardae_philox_normal_at", noise[at:], c * per_image, seed, offset, None, i0 * per_image)
                at += c * per_image
        elif self.toy:                                                          # one flat tensor [eps0 block | eps block]
            n0 = c * self.noise_blocks[0]
            noise[:n0].copy_(enc_noise[0][i0:i0 + c].reshape(-1))
            noise[n0:].copy_(enc_noise[1][i0:i0 + c].reshape(-1))
        else:                                                                   # rows [eps0 | eps]
            rows = noise.view(c * k, m._noise_width)
            rows[:, :m.noise_dim].copy_(enc_noise[0][i0:i0 + c].reshape(c * k, m.noise_dim))
            rows[:, m.noise_dim:].copy_(enc_noise[1][i0:i0 + c].reshape(c * k, m.z_dim))
        return noise

    # ---- evaluation ----------------------------------------------------------------------------------------------------------------
    def evaluate_rows(self, x_all, enc_noise=None, prop_noise=None):
        """The IWAE-k bound of every image, [N] on the device; nothing is read back.  An image whose sample covariance is not positive
        definite is NaN."""
        m, k, ke = self.model, self.k, self.ke
        N = x_all.size(0) if isinstance(x_all, torch.Tensor) and x_all.dim() else 0
        _check(x_all, "x_all", (max(N, 1), 1, m.input_dim))
        m._require_gpu(x_all)
        enc_noise, prop_noise = self._check_noise(N, enc_noise, prop_noise)
        x = x_all.view(N, m.input_dim)
        chunks = self.plan(N)
        with torch.no_grad():
            bufs = self._buffers(chunks[0][1] - chunks[0][0], x.device)
            seed = rng.get_state()["seed"]
            enc_offsets = [rng._next_offset() for _ in self.noise_blocks] if enc_noise is None else None
            prop_offset = rng._next_offset() if prop_noise is None else 0
            d, flat, packed, ws, zd = m._desc, m._flat, m._packed_weights(), bufs["ws"], m.z_dim
            out = torch.empty(N, device=x.device, dtype=torch.float32)
            for i0, i1 in chunks:
                c = i1 - i0
                xc = x[i0:i1]
                noise = self._chunk_noise(bufs, i0, c, enc_noise, seed, enc_offsets)
                L.call("ardae_model_encode", d, flat, packed, xc, noise, c, ke, ws, ws.numel(), bufs["zs"])
                L.call("ardae_iwae_proposal", bufs["zs"], None if prop_noise is None else prop_noise[i0:i1], c, ke, k, zd, self.jitter, seed, prop_offset,
                       i0 * k * zd, bufs["newz"], bufs["logq"], None, None, None)
                L.call("ardae_model_decode", d, flat, packed, bufs["newz"], c * k, ws, ws.numel(), bufs["out0"], bufs["out1"])
                L.call("ardae_model_loss_rows", d, bufs["out0"], bufs["out1"], xc, bufs["newz"], c * k, k, bufs["rec"], bufs["pri"])
                L.call("ardae_iwae_reduce", bufs["rec"], bufs["pri"], bufs["logq"], c, k, out[i0:i1])
        return out

    def evaluate(self, x_all, enc_noise=None, prop_noise=None):
        """Mean IWAE-k bound over the images of x_all (evaluate_iws' `logprob / num_total`); one host synchronisation."""
        rows = self.evaluate_rows(x_all, enc_noise, prop_noise)
        finite, mean = torch.stack([torch.isfinite(rows).all().double(), rows.double().mean()]).tolist()
        if not finite:
            raise ValueError(NOT_PD)
        return mean
