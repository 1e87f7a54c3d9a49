"""MI355X-native engine for the AR-DAE-VAE inner training loop (reference: ivae_ardae.py:546-846).

Drop-in surface (same names as the reference's `models` / `utils` re-exports used by ivae_ardae.py):
    MNISTIPVAE, ToyIPVAE, ToyAuxIPVAE, ConvIPVAE, MNISTAuxIPVAE, MNISTConvAuxIPVAE, ResConvIPVAE, MNISTResConvAuxIPVAE, MNISTResConvAuxIPVAEClipped, MLPGradCARDAE, MLPResCARDAE, MLPGradARDAE, MLPResARDAE, MLPGradDAE, MLPResDAE, MLPGradCDAE, MLPResCDAE, MLPDAE, MLPCDAE, Adam, RMSprop, normal_energy_func, annealing_func,
    Polyak, SWA (torchcontrib.optim wrappers of --m-weight-avg: use_buf() / use_sgd() around an evaluation)
Fused path:
    ArdaeEngine, TrainConfig  -- one train step as a straight line of C-ABI calls (what bench.py times)
    ArdaeScoreEngine, ScoreConfig -- the AR-DAE update of an unconditional score network (notebooks/ardae_toy.ipynb, ardae_fit.ipynb) as one captured unit
    ArdaeScoreEngine, DaeConfig -- the same engine on a plain DAE (MLPGradDAE / MLPResDAE) with notebooks/dae_toy.ipynb's annealed noise level
    ArdaeCondScoreEngine, ScoreConfig | DaeConfig -- the cDAE update of ivae_ardae.py:752-779 on samples of the caller's own amortised sampler as one captured unit, for a conditional
                                 AR-DAE (MLPGradCARDAE / MLPResCARDAE) or a plain conditional DAE (MLPGradCDAE / MLPResCDAE); score() = the entropy gradient of :826-834
    ArdaeScoreEngine | ArdaeCondScoreEngine, DaeConfig -- the same two engines on the reconstruction DAEs of models/dae/mlp.py (MLPDAE; MLPCDAE): gaussian or uniform noise at the
                                 annealed level, loss = mse(x_recon, x) through the same loss layer; score() = (x_recon - x) / sigma^2
    ArdaeFitEngine, FitConfig, Generator, energy -- a whole iteration of notebooks/ardae_fit.ipynb (implicit generator fitted to an energy function, the
                                 AR-DAE score as its entropy gradient) as one captured unit; utils/energy.py's functions on the device
    IwaeEvaluator, ArdaeEngine.evaluate_iws -- evaluate_iws of the recipes: the IWAE bound of a whole set in large chunks, the proposal fused into one
                                 kernel, one host synchronisation per set
    PosteriorDiagnostics, ArdaeEngine.diagnostics -- the visualisation block's numbers (ivae_ardae.py:952-1111): 2-D histograms of the latents at
                                 every noise level from one sampler pass, the data-recon-gen histograms of the 2-D problems, log var q(z); all on
                                 the device, one host synchronisation per pass
    MNISTVAE, ToyVAE, MNISTConvVAE, MNISTResConvVAE, MNISTAuxVAE, ToyAuxVAE, MNISTConvAuxVAE, MNISTResConvAuxVAE, VaeEngine, VaeConfig, GaussianIwaeEvaluator -- the Gaussian-posterior baselines of the reference's second trainer, vae.py
                                 (`--model mnist` / `--model toy` / `--model conv` / `--model resconv` / `--model auxmnist` / `--model auxtoy` / `--model auxconv`): drop-in modules, one iteration of its loop as one captured unit with the posterior
                                 draw, the reparameterisation and the analytic KL fused into the head kernel, and its evaluate_iws under the analytic posterior
    GaussianDiagnostics, VaeEngine.diagnostics, PosteriorDiagnostics.final_pass -- vae.py's visualisation block for the Gaussian baselines (2-D histograms
                                 of the latents of model(x), data | recon | gen of the 2-D problems; no host synchronisation) and both scripts' last
                                 block, the 256-bin heat maps of 1 000 000 points, through ardae_hist2d_wide (tables of up to 512 bins, cut into bands)
    ScalarLog                 -- the reference's per-step scalars through a device ring buffer (no host sync in the step)
The compute is libardae_hip.so (hand-written HIP for gfx950, C ABI in include/ardae_hip.h); there is no fallback.
"""
from . import _lib  # noqa: F401
from . import rng  # noqa: F401
from . import data  # noqa: F401
from . import energy  # noqa: F401
from .rng import manual_seed  # noqa: F401
from .modules import (MNISTIPVAE, ToyIPVAE, ToyAuxIPVAE, ConvIPVAE, MNISTAuxIPVAE, MNISTConvAuxIPVAE, ResConvIPVAE, MNISTResConvAuxIPVAE, MNISTResConvAuxIPVAEClipped, MLPGradCARDAE, MLPResCARDAE, MLPGradARDAE, MLPResARDAE, MLPGradDAE, MLPResDAE, MLPGradCDAE, MLPResCDAE, MLPDAE, MLPCDAE, ReconDAE, ReconConditionalDAE, ARDAE, DAE, ConditionalDAE, Generator, ImplicitPosteriorVAE, ConditionalARDAE,  # noqa: F401
                      normal_energy_func, GaussianVAE, MNISTVAE, ToyVAE, MNISTConvVAE, MNISTResConvVAE, MNISTAuxVAE, ToyAuxVAE, MNISTConvAuxVAE, MNISTResConvAuxVAE)
from .optim import Adam, RMSprop, Polyak, SWA  # noqa: F401
from .engine import ArdaeEngine, TrainConfig, annealing_func  # noqa: F401
from .score_engine import ArdaeCondScoreEngine, ArdaeScoreEngine, DaeConfig, ScoreConfig, dae_sigma  # noqa: F401
from .fit import ArdaeFitEngine, FitConfig  # noqa: F401
from .iwae import IwaeEvaluator, plan_chunks  # noqa: F401
from .diagnostics import PosteriorDiagnostics  # noqa: F401
from .vae import GaussianIwaeEvaluator, VaeConfig, VaeEngine  # noqa: F401
from .vae_diagnostics import GaussianDiagnostics  # noqa: F401
from .scalar_log import ScalarLog  # noqa: F401
