"""Host-side mirror of the reference's model / cDAE object surface, backed by the HIP library.

    net.MNISTIPVAE / net.ToyIPVAE        <- models/ivae/mnist.py:201-301, models/ivae/toy.py:739-873 (enc_type='concat')
    net.MLPGradCARDAE / net.MLPResCARDAE <- models/graddae/mlp.py:341-483, models/resdae/mlp.py:286-413
    net.MLPGradARDAE / net.MLPResARDAE   <- models/graddae/mlp.py:118-207, models/resdae/mlp.py:92-167
    net.MLPGradDAE / net.MLPResDAE       <- models/graddae/mlp.py:39-116, models/resdae/mlp.py:27-90
    net.MLPGradCDAE / net.MLPResCDAE     <- models/graddae/mlp.py:210-339, models/resdae/mlp.py:170-284
    net.MLPDAE / net.MLPCDAE             <- models/dae/mlp.py:21-82, :85-193 (the reconstruction DAEs: gaussian or uniform noise)
    net.MNISTVAE / net.ToyVAE            <- models/vae/mnist.py:99-220, models/vae/toy.py:99-213 (the Gaussian-posterior baselines of vae.py)
    net.MNISTConvVAE                     <- models/vae/conv.py:138-260 (`vae.py --model conv`)
    net.MNISTResConvVAE                  <- models/vae/resconv.py:122-240 (`vae.py --model resconv`)
    net.MNISTAuxVAE / net.ToyAuxVAE      <- models/vae/auxmnist.py:268-451, models/vae/auxtoy.py (`vae.py --model auxmnist | auxtoy`)

Same constructor kwargs, same `state_dict()` keys and `[out, in]` layouts (reference checkpoints load), same method
names and argument meaning, same exception types.  Parameters are `nn.Parameter` views into ONE flat fp32 buffer
(the layout the C ABI consumes); forward/backward are `torch.autograd.Function`s that call the ABI.  There is no
PyTorch fallback: on a CPU tensor or without the built library these modules raise.
"""
import math
import weakref

import torch
import torch.nn as nn

from . import _lib as L
from . import layout
from . import rng


class _Box(nn.Module):
    """Name-only container (gives parameters their dotted reference names)."""


class _EncodeBox(_Box):
    """`model.encode(x, std=0)` -> [B, nz, z] (Encoder.forward, ivae/mnist.py:102-121).  Holds the `encode.*` parameters by
    name; the computation is the owning model's sampler (the owner is kept out of the module tree on purpose)."""

    def forward(self, x, noise=None, std=None, nz=1):
        o = self._owner_ref()
        return o._sample(o._x(x), nz, std, noise)

    def forward_hidden(self, x, std=None, nz=1):
        """Aux models: `model.encode.forward_hidden(x, std=0)` -> cat(h0, h) [B, 2 h], the `hidden1a` cDAE context
        (ivae/auxmnist.py:125-132, ivae_ardae.py:737-739)."""
        assert nz == 1                                    # ivae/auxmnist.py:126
        if std is None or float(std) != 0.0:
            raise NotImplementedError("forward_hidden is implemented for std=0 (its only use in ivae_ardae.py)")
        return self._owner_ref()._hidden(x)


class FlatParamModule(nn.Module):
    _no_grad_names = frozenset()     # parameters that receive no gradient (and keep no optimiser state)

    def _build_params(self, spec, boxes=None):
        boxes = boxes or {}
        self._spec = spec
        self._offs, total = layout.offsets(spec)
        self.register_buffer("_flat", torch.zeros(total), persistent=False)
        for name, (off, n, shape) in self._offs.items():
            parts = name.split(".")
            mod = self
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, boxes.get(p, _Box)() if mod is self else _Box())
                mod = mod._modules[p]
            par = nn.Parameter(self._flat[off:off + n].view(shape))
            par._ardae_owner = weakref.ref(self)          # net.Adam / net.RMSprop find the owning module through it (optim.py)
            mod.register_parameter(parts[-1], par)
        self._packed = None
        self._tracked = False        # see _pack_is_current
        self._packed_ver = None

    # Weight image policy of the module path.  Default: re-pack at EVERY use (one launch over ~2-12 MB), because tensor version
    # counters cannot be trusted to see an update - `p.data.add_(...)`, which is how the reference's vendored Adam writes
    # (utils/optim.py:106), bumps none - so any optimiser, the reference's included, may be used with these modules.  Once one of
    # THIS package's optimisers (optim.py: they bump the counters) is built over the parameters the module switches to tracking:
    # the image is rebuilt only when a parameter's version has moved (optimiser step, load_state_dict, any in-place op on p).
    # Writing through `p.data` by hand in that mode needs `mark_dirty()`.
    def _pack_is_current(self):
        if self._packed is None or not self._tracked:
            return False
        return self._packed_ver == tuple(p._version for p in self.parameters())

    def _note_packed(self):
        self._packed_ver = tuple(p._version for p in self.parameters())

    def mark_dirty(self):
        """Parameters were written behind autograd's back (`p.data...`) while one of net's optimisers tracks them."""
        self._packed_ver = None

    # keep the parameters views of the flat buffer across .to()/.cuda()/.float()
    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self._relink()
        return self

    def _relink(self):
        flat = self._flat
        for name, p in self.named_parameters():
            off, n, shape = self._offs[name]
            p.data = flat[off:off + n].view(shape)
        self._packed = None

    def flat_params(self):
        return self._flat

    def param_views(self, flat, grads_only=False):
        """A buffer laid out like `_flat` (gradients, optimiser state, an average) as per-parameter views in named_parameters() order;
        grads_only: None in the place of a parameter that receives no gradient."""
        return [None if grads_only and name in self._no_grad_names else flat[off:off + n].view(shape)
                for name, (off, n, shape) in ((name, self._offs[name]) for name, _ in self.named_parameters())]

    def _default_init(self):
        """nn.Linear's default init (kaiming_uniform(a=sqrt 5) == U(+-1/sqrt(fan_in)) for weight and bias)."""
        spec = dict(self._spec)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith(".scale") or name.endswith(".direction") or (name[:-len("bias")] + "direction") in spec:
                    continue                                        # weight-normalised operators: reset_parameters() of the owning model
                wshape = p.shape if name.endswith("weight") else spec[name[:-len("bias")] + "weight"]
                fan_in = wshape[1] * (wshape[2] * wshape[3] if len(wshape) == 4 else 1)   # torch's fan_in for (transposed) convs too
                bound = 1.0 / math.sqrt(fan_in)
                p.uniform_(-bound, bound)

    def _require_gpu(self, *tensors):
        if not self._flat.is_cuda:
            raise RuntimeError(f"{type(self).__name__}: parameters are on {self._flat.device}; the HIP engine needs .to('cuda') "
                               "(there is no CPU path)")
        for t in tensors:
            if t is not None and not t.is_cuda:
                raise RuntimeError(f"{type(self).__name__}: got a {t.device} tensor; inputs must be on the GPU")

    def _ws(self, nfloats):
        return torch.empty(nfloats, device=self._flat.device, dtype=torch.float32)

    _packed_floats_fn = _pack_fn = None      # the network family's two entry points (ardae_cdae_* | ardae_model_* | ardae_gen_*), which
    _abi = None                              # take the network as `*self._abi`: (descriptor,), the generator's five integers

    def _packed_weights(self):
        """MFMA-lane-linear image of the current weights (policy: _pack_is_current; the fused engine keeps its own image and re-packs
        right after its own optimiser kernels)."""
        if self._pack_is_current():
            return self._packed
        if self._packed is None:
            self._packed = self._ws(L.query(self._packed_floats_fn, *self._abi))
        L.call(self._pack_fn, *self._abi, self._flat, self._packed)
        self._note_packed()
        return self._packed


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


KIND_IDS = {"mnist": 0, "toy": 1, "conv": 2, "auxmnist": 3, "auxconv": 4, "resconv": 5, "auxresconv": 6, "auxtoy": 7,      # ardae_model_desc.kind
            "vae_mnist": 8, "vae_toy": 9, "vae_conv": 11, "vae_resconv": 12,                                                    # (vae.py's baselines: GaussianVAE below; 10 is not a kind)
            "vae_auxmnist": 14, "vae_auxtoy": 15,                                                                               # (its auxiliary-variable baselines; 13 is not a kind)
            "vae_auxconv": 17,                                                                                                  # (16 is not a kind)
            "vae_auxresconv": 19}                                                                                               # (18 is not a kind)
AUX_KINDS = ("auxmnist", "auxconv", "auxresconv", "auxtoy")                                                 # hierarchical samplers
GAUSSIAN_DECODERS = ("toy", "auxtoy", "vae_toy", "vae_auxtoy")                                                                     # decode.reparam.{mean_fn, logvar_fn}


# ---------------------------------------------------------------------------------------------------------------
# AR-DAE score networks: conditional (the cDAE of ivae_ardae.py) and unconditional (notebooks/ardae_toy.ipynb / ardae_fit.ipynb)
# ---------------------------------------------------------------------------------------------------------------
class _ArdaeLossFn(torch.autograd.Function):
    """forward = the loss of ConditionalARDAE.forward / ARDAE.forward (context None, S = 1); the double backward runs in the same ABI
    call, so backward() only scales."""

    @staticmethod
    def forward(ctx, mod, xbar, sigma, eps, context, B, S, *params):
        d = mod._desc
        ws = mod._ws(L.query("ardae_cdae_workspace_floats", d, B, S, 1))
        loss = torch.empty(1, device=xbar.device)
        grads = torch.zeros_like(mod._flat)
        L.call("ardae_cdae_loss_grads", d, mod._flat, mod._packed_weights(), xbar, sigma, eps, context, B, S, ws, ws.numel(), loss, grads, None)
        ctx.mod, ctx.grads = mod, grads
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        # (no gradient: the reference leaves .grad = None there - the energy's offset does not reach its input-gradient)
        return (None,) * 7 + tuple(None if g is None else g * gloss for g in ctx.mod.param_views(ctx.grads, grads_only=True))


class _ScoreNet(FlatParamModule):
    """What ConditionalARDAE and ARDAE share: the constructor checks, the ardae_cdae_desc and the parameter buffer."""
    _kind = None                 # "grad" | "res": the leaf classes
    _packed_floats_fn, _pack_fn = "ardae_cdae_packed_floats", "ardae_cdae_pack"

    @staticmethod
    def _check(noise_type, nonlinearity, also=None):
        if noise_type != "gaussian":
            raise NotImplementedError            # uniform / laplace (graddae/mlp.py:143-146,392-393) are not on the path
        if also:
            raise NotImplementedError(also)
        if nonlinearity not in L.ACT or nonlinearity in ("none", None):
            raise NotImplementedError(f"nonlinearity {nonlinearity!r}: get_nonlinear_func (utils/models.py:14-32) knows relu, softplus / csoftplus, elu, tanh, leaky_relu and swish")

    def _build_net(self, first_kind, spec, input_dim, context_dim, h_dim, std, num_hidden_layers, nonlinearity, noise_type):
        """first_kind: ardae_cdae_desc.kind of the grad class (0 conditional, 2 unconditional, 6 plain DAE, 10 plain conditional DAE, 16 conditional
        without an input encoder); its res sibling is the next."""
        self.input_dim, self.h_dim, self.std = input_dim, h_dim, std
        self.num_hidden_layers, self.nonlinearity, self.noise_type = num_hidden_layers, nonlinearity, noise_type
        self._desc = L.CdaeDesc(first_kind if self._kind == "grad" else first_kind + 1, input_dim, context_dim, h_dim, num_hidden_layers, L.ACT[nonlinearity])
        self._abi = (self._desc,)
        self._build_params(spec)
        if self._kind == "grad":
            self._no_grad_names = frozenset({"neglogprob.fc.bias"})
        self._default_init()


class ConditionalARDAE(_ScoreNet):
    def __init__(self, input_dim=2, h_dim=128, context_dim=2, std=0.01, num_hidden_layers=1, nonlinearity="tanh",
                 noise_type="gaussian", enc_input=True, enc_ctx=True, std_method="default"):
        super().__init__()
        self._check(noise_type, nonlinearity, None if enc_ctx else
                    "enc_ctx=False is not built: the last MLP would read the raw concatenation [input | context | std] "
                    "(enc_input may be False: ardae_cdae_desc.kind 16 / 17)")
        self.context_dim, self.enc_input, self.enc_ctx = context_dim, bool(enc_input), enc_ctx
        # enc_input=True: what ivae_ardae.py:583-606 constructs (kind 0 / 1); False: the last MLP reads the perturbed sample itself (kind 16 / 17)
        self._build_net(0 if enc_input else 16, layout.cdae_spec(self._kind, input_dim, context_dim, h_dim, num_hidden_layers, bool(enc_input)),
                        input_dim, context_dim, h_dim, std, num_hidden_layers, nonlinearity, noise_type)

    def _prep(self, input, context, std):
        assert input.dim() == 3      # bsz x ssz x x_dim   (graddae/mlp.py:402)
        assert context.dim() == 3    # bsz x 1 x ctx_dim   (graddae/mlp.py:403)
        B, S = input.size(0), input.size(1)
        self._require_gpu(input, context)
        if std is None:
            std = input.new_zeros(B, S, 1)
        else:
            assert torch.is_tensor(std)
        x = _f32c(input).view(B * S, self.input_dim)
        c = _f32c(context).view(B, self.context_dim)
        s = _f32c(std).reshape(B * S)
        return B, S, x, c, s

    def forward(self, input, context, std=None, scale=None, eps=None):
        """-> (None, loss) like the reference.  `scale` is accepted and ignored (graddae/mlp.py:410-411).
        `eps` injects the Gaussian perturbation draw ([B*S, x_dim]); default: the library's Philox stream."""
        B, S, x, c, s = self._prep(input, context, std)
        if eps is None:
            eps = rng.normal((B * S, self.input_dim), x.device)
        eps = _f32c(eps).view(B * S, self.input_dim)
        xbar = torch.addcmul(x, s[:, None], eps)         # add_gaussian_noise (graddae/mlp.py:21-23)
        loss = _ArdaeLossFn.apply(self, xbar, s, eps, c, B, S, *self.parameters())
        return None, loss

    def glogprob(self, input, context, std=None, scale=None):
        B, S, x, c, s = self._prep(input, context, std)
        ws = self._ws(L.query("ardae_cdae_workspace_floats", self._desc, B, S, 0))
        out = torch.empty(B * S, self.input_dim, device=x.device)
        L.call("ardae_cdae_score", self._desc, self._flat, self._packed_weights(), x, s, c, B, S, ws, ws.numel(), out)
        return out.view(B, S, self.input_dim)


class MLPGradCARDAE(ConditionalARDAE):
    """models/graddae/mlp.py::ConditionalARDAE (`--cdae mlp-grad`)."""
    _kind = "grad"


class MLPResCARDAE(ConditionalARDAE):
    """models/resdae/mlp.py::ConditionalARDAE (`--cdae mlp-res`)."""
    _kind = "res"


class ConditionalDAE(_ScoreNet):
    """models/graddae/mlp.py:210-339 / models/resdae/mlp.py:170-284: the conditional score network that is not amortised over the noise level -
    ConditionalARDAE without the sigma input: one noise level per call (`std`, default `self.std`), not an input of the network."""

    def __init__(self, input_dim=2, h_dim=128, context_dim=2, std=0.01, num_hidden_layers=1, nonlinearity="tanh", noise_type="gaussian",
                 enc_input=True, enc_ctx=True):
        super().__init__()
        self._check(noise_type, nonlinearity, None if enc_input and enc_ctx else
                    "enc_input=enc_ctx=True is the only configuration built (the sibling ConditionalARDAE's)")
        self.context_dim, self.enc_input, self.enc_ctx = context_dim, enc_input, enc_ctx
        self._build_net(10, layout.cdae_plain_spec(self._kind, input_dim, context_dim, h_dim, num_hidden_layers), input_dim, context_dim, h_dim,
                        std, num_hidden_layers, nonlinearity, noise_type)

    def _prep(self, input, context):
        assert input.dim() == 3      # bsz x ssz x x_dim   (graddae/mlp.py:271)
        assert context.dim() == 3    # bsz x 1 x ctx_dim   (graddae/mlp.py:272)
        B, S = input.size(0), input.size(1)
        self._require_gpu(input, context)
        return B, S, _f32c(input).view(B * S, self.input_dim), _f32c(context).view(B, self.context_dim)

    def forward(self, input, context, std=None, eps=None):
        """-> (None, loss) like the reference.  `std`: None (self.std), a Python number, or a tensor that broadcasts to [B*S, 1]
        (graddae/mlp.py:273,304).  `eps` injects the Gaussian perturbation draw ([B*S, x_dim]); default: the library's Philox stream."""
        B, S, x, c = self._prep(input, context)
        N = B * S
        std = self.std if std is None else std
        if torch.is_tensor(std):
            self._require_gpu(std)
            s = torch.broadcast_to(_f32c(std), (N, 1)).reshape(-1).contiguous()
        else:
            s = torch.full((N,), float(std), device=x.device, dtype=torch.float32)
        if eps is None:
            eps = rng.normal((N, self.input_dim), x.device)
        eps = _f32c(eps).view(N, self.input_dim)
        xbar = torch.empty_like(x)
        L.call("ardae_dae_perturb", x, s, eps, N, 1, self.input_dim, xbar)      # add_gaussian_noise (graddae/mlp.py:21-23)
        loss = _ArdaeLossFn.apply(self, xbar, s, eps, c, B, S, *self.parameters())
        return None, loss

    def glogprob(self, input, context, std=None):
        """The score at `input` given `context`; `std` is accepted and ignored, as in the reference (graddae/mlp.py:309-339)."""
        B, S, x, c = self._prep(input, context)
        ws = self._ws(L.query("ardae_cdae_workspace_floats", self._desc, B, S, 0))
        out = torch.empty(B * S, self.input_dim, device=x.device)
        L.call("ardae_cdae_score", self._desc, self._flat, self._packed_weights(), x, None, c, B, S, ws, ws.numel(), out)
        return out.view(B, S, self.input_dim)


class MLPGradCDAE(ConditionalDAE):
    """models/graddae/mlp.py::ConditionalDAE (exported as MLPGradCDAE, models/__init__.py:12): score = input-gradient of an energy MLP."""
    _kind = "grad"


class MLPResCDAE(ConditionalDAE):
    """models/resdae/mlp.py::ConditionalDAE (exported as MLPResCDAE, models/__init__.py:7): the MLP's output is the score."""
    _kind = "res"


class ARDAE(_ScoreNet):
    """models/graddae/mlp.py:118-207 / models/resdae/mlp.py:92-167: the AR-DAE score network on [x_bar | sigma], no context."""

    def __init__(self, input_dim=2, h_dim=1000, std=0.1, num_hidden_layers=1, nonlinearity="tanh", noise_type="gaussian"):
        super().__init__()
        self._check(noise_type, nonlinearity)
        if num_hidden_layers < 1:
            raise NotImplementedError("num_hidden_layers >= 1 (a score network without a hidden layer is linear in [x | sigma])")
        self._build_net(2, layout.dae_spec(self._kind, input_dim, h_dim, num_hidden_layers), input_dim, 0, h_dim, std, num_hidden_layers,
                        nonlinearity, noise_type)

    def _prep(self, input, std):
        self._require_gpu(input, std if torch.is_tensor(std) else None)
        batch_size = input.size(0)
        x = _f32c(input).view(-1, self.input_dim)
        if std is None:
            std = x.new_zeros(batch_size, 1)                # graddae/mlp.py:159-160
        else:
            assert torch.is_tensor(std)
        s = _f32c(std).reshape(-1)
        if s.numel() != x.size(0):
            raise ValueError(f"std has {s.numel()} entries for {x.size(0)} rows")
        return x, s

    def forward(self, input, std=None, eps=None):
        """-> (None, loss) like the reference.  `eps` injects the Gaussian perturbation draw ([N, input_dim]); default: the library's
        Philox stream."""
        x, s = self._prep(input, std)
        N = x.size(0)
        if eps is None:
            eps = rng.normal((N, self.input_dim), x.device)
        eps = _f32c(eps).view(N, self.input_dim)
        xbar = torch.empty_like(x)
        L.call("ardae_dae_perturb", x, s, eps, N, 1, self.input_dim, xbar)      # add_gaussian_noise (graddae/mlp.py:21-23)
        loss = _ArdaeLossFn.apply(self, xbar, s, eps, None, N, 1, *self.parameters())
        return None, loss

    def glogprob(self, input, std=None):
        x, s = self._prep(input, std)
        N = x.size(0)
        ws = self._ws(L.query("ardae_cdae_workspace_floats", self._desc, N, 1, 0))
        out = torch.empty(N, self.input_dim, device=x.device)
        L.call("ardae_cdae_score", self._desc, self._flat, self._packed_weights(), x, s, None, N, 1, ws, ws.numel(), out)
        return out


class MLPGradARDAE(ARDAE):
    """models/graddae/mlp.py::ARDAE (exported as MLPGradARDAE, models/__init__.py:11): score = input-gradient of an energy MLP."""
    _kind = "grad"


class MLPResARDAE(ARDAE):
    """models/resdae/mlp.py::ARDAE (exported as MLPResARDAE, models/__init__.py:6): the MLP's output is the score."""
    _kind = "res"


class DAE(_ScoreNet):
    """models/graddae/mlp.py:39-116 / models/resdae/mlp.py:27-90: the plain denoising autoencoder of notebooks/dae_toy.ipynb, a score network
    on x_bar alone - one noise level per call (`std`, default `self.std`), not an input of the network."""

    def __init__(self, input_dim=2, h_dim=1000, std=0.1, num_hidden_layers=1, nonlinearity="tanh", noise_type="gaussian"):
        super().__init__()
        self._check(noise_type, nonlinearity)
        if num_hidden_layers < 1:
            raise NotImplementedError("num_hidden_layers >= 1 (a score network without a hidden layer is linear in x)")
        self._build_net(6, layout.dae_plain_spec(self._kind, input_dim, h_dim, num_hidden_layers), input_dim, 0, h_dim, std, num_hidden_layers,
                        nonlinearity, noise_type)

    def _rows(self, input):
        self._require_gpu(input)
        return _f32c(input).view(-1, self.input_dim)

    def forward(self, input, std=None, eps=None):
        """-> (None, loss) like the reference.  `std`: None (self.std), a Python number, or a tensor that broadcasts to [N, 1]
        (graddae/mlp.py:77,96).  `eps` injects the Gaussian perturbation draw ([N, input_dim]); default: the library's Philox stream."""
        x = self._rows(input)
        N = x.size(0)
        std = self.std if std is None else std
        if torch.is_tensor(std):
            self._require_gpu(std)
            s = torch.broadcast_to(_f32c(std), (N, 1)).reshape(-1).contiguous()
        else:
            s = torch.full((N,), float(std), device=x.device, dtype=torch.float32)
        if eps is None:
            eps = rng.normal((N, self.input_dim), x.device)
        eps = _f32c(eps).view(N, self.input_dim)
        xbar = torch.empty_like(x)
        L.call("ardae_dae_perturb", x, s, eps, N, 1, self.input_dim, xbar)      # add_gaussian_noise (graddae/mlp.py:21-23)
        loss = _ArdaeLossFn.apply(self, xbar, s, eps, None, N, 1, *self.parameters())
        return None, loss

    def glogprob(self, input, std=None):
        """The score at `input`; `std` is accepted and ignored, as in the reference (graddae/mlp.py:101-116)."""
        x = self._rows(input)
        N = x.size(0)
        ws = self._ws(L.query("ardae_cdae_workspace_floats", self._desc, N, 1, 0))
        out = torch.empty(N, self.input_dim, device=x.device)
        L.call("ardae_cdae_score", self._desc, self._flat, self._packed_weights(), x, None, None, N, 1, ws, ws.numel(), out)
        return out


class MLPGradDAE(DAE):
    """models/graddae/mlp.py::DAE (exported as MLPGradDAE, models/__init__.py): score = input-gradient of an energy MLP on x_bar."""
    _kind = "grad"


class MLPResDAE(DAE):
    """models/resdae/mlp.py::DAE (exported as MLPResDAE, models/__init__.py): the MLP's output is the score."""
    _kind = "res"


# ---------------------------------------------------------------------------------------------------------------
# The reconstruction DAEs of models/dae/mlp.py: x_recon = net(x_bar), loss = mse(x_recon, x), score = (net(x) - x) / std^2
# ---------------------------------------------------------------------------------------------------------------
class _ReconLossFn(torch.autograd.Function):
    """forward = (loss, x_recon) of DAE.forward / ConditionalDAE.forward (dae/mlp.py:54-70,136-165) on a given x_bar: the res kinds' loss
    layer on (x_bar, ones, -x) - rho = 1 * y + (-x) is y - x exactly - with the network's output taken as score_out.  The backward runs in
    the same ABI call, so backward() only scales; x_recon carries no gradient."""

    @staticmethod
    def forward(ctx, mod, xbar, ones, target, context, B, S, *params):
        d = mod._desc
        ws = mod._ws(L.query("ardae_cdae_workspace_floats", d, B, S, 1))
        loss = torch.empty(1, device=xbar.device)
        grads = torch.zeros_like(mod._flat)
        recon = torch.empty_like(xbar)
        L.call("ardae_cdae_loss_grads", d, mod._flat, mod._packed_weights(), xbar, ones, target, context, B, S, ws, ws.numel(), loss, grads, recon)
        ctx.mod, ctx.grads = mod, grads
        ctx.mark_non_differentiable(recon)
        return loss.reshape(()), recon

    @staticmethod
    def backward(ctx, gloss, _grecon):
        return (None,) * 7 + tuple(g * gloss for g in ctx.mod.param_views(ctx.grads))


class _ReconNet(_ScoreNet):
    """What ReconDAE and ReconConditionalDAE share: the refusals, add_noise, and the two calls around the network."""
    _kind = "res"                # the network's output is a point of the input space: the res kinds' networks (kind 7 / 11 / 13)
    _recon = True                # the engines tell a reconstruction DAE from a residual one by this: the network kind cannot
    NOISE = {"gaussian": 0, "uniform": 1}      # ardae_recon_perturb's `noise`

    @classmethod
    def _check_recon(cls, noise_type, nonlinearity, num_hidden_layers, also=None):
        if noise_type not in cls.NOISE:
            raise NotImplementedError(f"noise_type {noise_type!r}: add_noise (dae/mlp.py:40-47) knows 'gaussian' and 'uniform'")
        cls._check("gaussian", nonlinearity, also)
        if num_hidden_layers < 1:
            raise NotImplementedError("num_hidden_layers >= 1 (without a hidden layer the denoiser is linear in its input)")

    def add_noise(self, input, std=None, eps=None):
        """x_bar of dae/mlp.py:12-18,40-47 for rows [N, d].  `eps`: the raw draw [N, d] - standard normals, or uniforms in [0, 1); default: the
        library's Philox stream."""
        return self._perturb(_f32c(input).view(-1, self.input_dim), std, eps)[0]

    def _perturb(self, x, std, eps):
        """-> x_bar, ones [N], -x: what the loss layer reads.  std: None (self.std), a Python number, or a tensor that broadcasts to [N, 1]."""
        N, d, noise = x.size(0), self.input_dim, self.NOISE[self.noise_type]
        std = self.std if std is None else std
        if eps is None:
            eps = (rng.uniform if noise else rng.normal)((N, d), x.device)
        eps = _f32c(eps).view(N, d)
        xbar = torch.empty_like(x)
        if not torch.is_tensor(std):
            ones, target = torch.empty(N, device=x.device), torch.empty_like(x)
            L.call("ardae_recon_perturb", x, eps, N, 1, d, noise, float(std), None, xbar, ones, target)
            return xbar, ones, target
        # a noise level per row (ardae_recon_perturb takes one per call): the same expressions, row by row
        self._require_gpu(std)
        s = torch.broadcast_to(_f32c(std), (N, 1)).contiguous()
        if noise:
            xbar = x + ((2.0 * s) * eps - s)                                        # add_uniform_noise (dae/mlp.py:16-18), its order
        else:
            L.call("ardae_dae_perturb", x, s.view(N), eps, N, 1, d, xbar)           # add_gaussian_noise (dae/mlp.py:12-14)
        return xbar, torch.ones(N, device=x.device), -x

    def _residual_score(self, recon, x, std):
        """(recon - x) / std^2 (dae/mlp.py:80-81), in place of recon"""
        std = self.std if std is None else std
        if torch.is_tensor(std):
            self._require_gpu(std)
            return (recon - x) / torch.broadcast_to(_f32c(std), (x.size(0), 1)) ** 2
        L.call("ardae_recon_score", recon, x, x.size(0), self.input_dim, float(std), None, recon)
        return recon


class ReconDAE(_ReconNet):
    """models/dae/mlp.py:21-82 (exported as MLPDAE): the classical denoising autoencoder, `main = MLP(d, h, d)` - the network of MLPResDAE."""

    def __init__(self, input_dim=2, h_dim=1000, std=0.1, num_hidden_layers=1, nonlinearity="tanh", noise_type="gaussian"):
        super().__init__()
        self._check_recon(noise_type, nonlinearity, num_hidden_layers)
        self._build_net(6, layout.dae_plain_spec("res", input_dim, h_dim, num_hidden_layers), input_dim, 0, h_dim, std, num_hidden_layers,
                        nonlinearity, noise_type)

    def forward(self, input, std=None, eps=None):
        """-> (x_recon [N, d], loss) like the reference (dae/mlp.py:54-70).  x_recon is returned DETACHED (the reference's is attached to the
        graph); loss is differentiable with respect to the parameters.  `std`: None (self.std), a Python number, or a tensor that broadcasts
        to [N, 1].  `eps` injects the raw draw [N, d]: normals, or uniforms in [0, 1); default: the library's Philox stream."""
        self._require_gpu(input)
        x = _f32c(input).view(-1, self.input_dim)
        xbar, ones, target = self._perturb(x, std, eps)
        loss, recon = _ReconLossFn.apply(self, xbar, ones, target, None, x.size(0), 1, *self.parameters())
        return recon, loss

    def glogprob(self, input, std=None):
        """(main(x) - x) / std^2, in the shape of `input` (dae/mlp.py:72-82)."""
        self._require_gpu(input)
        x = _f32c(input).view(input.size(0), self.input_dim)
        N = x.size(0)
        ws = self._ws(L.query("ardae_cdae_workspace_floats", self._desc, N, 1, 0))
        out = torch.empty(N, self.input_dim, device=x.device)
        L.call("ardae_cdae_score", self._desc, self._flat, self._packed_weights(), x, None, None, N, 1, ws, ws.numel(), out)
        return self._residual_score(out, x, std).view(input.size())


class MLPDAE(ReconDAE):
    """models/dae/mlp.py::DAE (exported as MLPDAE, models/__init__.py)."""


class ReconConditionalDAE(_ReconNet):
    """models/dae/mlp.py:85-193 (exported as MLPCDAE): the conditional denoising autoencoder.  `context` is [B, S, c], one context row PER SAMPLE
    ROW (:146), so the ABI is called with B = N, S = 1; a [B, 1, c] tensor expanded along dim 1 (stride 0 there) is one context per image and
    runs as (B, S).  enc_input=False (the default): the last MLP reads x_bar beside the encoded context (ardae_cdae_desc.kind 13);
    enc_input=True: MLPResCDAE's network (kind 11)."""

    def __init__(self, input_dim=2, h_dim=128, context_dim=2, std=0.1, num_hidden_layers=1, nonlinearity="tanh", noise_type="gaussian",
                 enc_input=False, enc_ctx=True):
        super().__init__()
        self._check_recon(noise_type, nonlinearity, num_hidden_layers, None if enc_ctx else
                          "enc_ctx=False is not built: the last MLP would read the raw concatenation [x | ctx]")
        self.context_dim, self.enc_input, self.enc_ctx = context_dim, enc_input, enc_ctx
        self._build_net(10 if enc_input else 12, layout.recon_cdae_spec(input_dim, context_dim, h_dim, num_hidden_layers, enc_input), input_dim,
                        context_dim, h_dim, std, num_hidden_layers, nonlinearity, noise_type)

    def _prep(self, input, context):
        """-> (B, S) of the ABI call, x [N, d], ctx [B, c]"""
        assert input.dim() == 3      # bsz x ssz x x_dim     (dae/mlp.py:138)
        assert context.dim() == 3    # bsz x ssz x ctx_dim   (dae/mlp.py:139)
        self._require_gpu(input, context)
        B, S = input.size(0), input.size(1)
        if tuple(context.shape) != (B, S, self.context_dim):
            raise ValueError(f"context must be [{B}, {S}, {self.context_dim}] (one row per sample row), got {list(context.shape)}")
        x = _f32c(input).view(B * S, self.input_dim)
        if S > 1 and context.stride(1) == 0:               # one context per image, expanded over its samples
            return B, S, x, _f32c(context[:, 0, :])
        return B * S, 1, x, _f32c(context).view(B * S, self.context_dim)

    def forward(self, input, context, std=None, eps=None):
        """-> (x_recon [N, d], loss) like the reference (dae/mlp.py:136-165).  x_recon is returned DETACHED (the reference's is attached to the
        graph); loss is differentiable with respect to the parameters.  `std`: None (self.std), a Python number, or a tensor that broadcasts
        to [N, 1].  `eps` injects the raw draw [N, d]: normals, or uniforms in [0, 1); default: the library's Philox stream."""
        B, S, x, c = self._prep(input, context)
        xbar, ones, target = self._perturb(x, std, eps)
        loss, recon = _ReconLossFn.apply(self, xbar, ones, target, c, B, S, *self.parameters())
        return recon, loss

    def glogprob(self, input, context, std=None):
        """(dae(x, ctx) - x) / std^2 -> [B, S, d] (dae/mlp.py:167-193)."""
        B, S, x, c = self._prep(input, context)
        ws = self._ws(L.query("ardae_cdae_workspace_floats", self._desc, B, S, 0))
        out = torch.empty(B * S, self.input_dim, device=x.device)
        L.call("ardae_cdae_score", self._desc, self._flat, self._packed_weights(), x, None, c, B, S, ws, ws.numel(), out)
        return self._residual_score(out, x, std).view(input.size())


class MLPCDAE(ReconConditionalDAE):
    """models/dae/mlp.py::ConditionalDAE (exported as MLPCDAE, models/__init__.py)."""


# ---------------------------------------------------------------------------------------------------------------
# The implicit generator of notebooks/ardae_fit.ipynb
# ---------------------------------------------------------------------------------------------------------------
class _GenFn(torch.autograd.Function):
    """x = main(z) through ardae_gen_forward; backward = ardae_gen_backward on the incoming seed (the workspace keeps the hidden layers, so
    the notebook's two backward calls through one forward - retain_graph=True - both work)."""

    @staticmethod
    def forward(ctx, mod, z, *params):
        B = z.size(0)
        ws = mod._ws(L.query("ardae_gen_workspace_floats", *mod._net, B))
        x = torch.empty(B, mod.input_dim, device=z.device, dtype=torch.float32)
        L.call("ardae_gen_forward", *mod._net, mod._flat, mod._packed_weights(), z, B, ws, ws.numel(), x)
        ctx.mod, ctx.z, ctx.ws = mod, z, ws
        return x

    @staticmethod
    def backward(ctx, dx):
        mod = ctx.mod
        grads = torch.zeros_like(mod._flat)
        L.call("ardae_gen_backward", *mod._net, mod._flat, mod._packed_weights(), ctx.z, _f32c(dx), ctx.z.size(0), ctx.ws, ctx.ws.numel(), grads)
        return (None, None) + tuple(mod.param_views(grads))


class Generator(FlatParamModule):
    """notebooks/ardae_fit.ipynb `Generator`: main = Linear(z_dim, h) -> act -> [Linear(h, h) -> act] x (num_hidden_layers - 1) ->
    Linear(h, input_dim); the notebook's is num_hidden_layers=3, nonlinearity='relu'.  state_dict() keys are the nn.Sequential's,
    main.{0, 2, 4, ...}.{weight, bias}.  `energy_func`: what `loss` averages (the notebook reads a global; default net.energy.energy_func4,
    the notebook's choice)."""

    _packed_floats_fn, _pack_fn = "ardae_gen_packed_floats", "ardae_gen_pack"

    def __init__(self, input_dim=2, hidden_dim=64, z_dim=2, num_hidden_layers=3, nonlinearity="relu", energy_func=None):
        super().__init__()
        if nonlinearity not in L.ACT or nonlinearity in ("none", None):
            raise NotImplementedError(f"nonlinearity {nonlinearity!r}: get_nonlinear_func (utils/models.py:14-32) knows relu, softplus / csoftplus, elu, tanh, leaky_relu and swish")
        if not (int(input_dim) >= 1 and int(hidden_dim) >= 1 and int(z_dim) >= 1 and 1 <= int(num_hidden_layers) <= 16):
            raise ValueError(f"Generator: dimensions must be positive and 1 <= num_hidden_layers <= 16 (got input_dim={input_dim}, hidden_dim={hidden_dim}, "
                             f"z_dim={z_dim}, num_hidden_layers={num_hidden_layers})")
        self.input_dim, self.hidden_dim, self.z_dim = int(input_dim), int(hidden_dim), int(z_dim)
        self.num_hidden_layers, self.nonlinearity = int(num_hidden_layers), nonlinearity
        if energy_func is None:
            from . import energy
            energy_func = energy.energy_func4
        self.energy_func = energy_func
        # the network as the ABI takes it: z_dim, h_dim, n_layers, out_dim, act
        self._net = self._abi = (self.z_dim, self.hidden_dim, self.num_hidden_layers, self.input_dim, L.ACT[nonlinearity])
        self._build_params(layout.gen_spec(self.input_dim, self.hidden_dim, self.z_dim, self.num_hidden_layers))
        self._default_init()

    def sample_noise(self, batch_size):
        """[batch_size, z_dim] standard normals from the library's host Philox stream."""
        self._require_gpu()
        return rng.normal((int(batch_size), self.z_dim), self._flat.device)

    def loss(self, x):
        return torch.mean(self.energy_func(x))

    def forward(self, batch_size=None, z=None):
        """-> (x, loss) like the notebook's.  `z` injects the noise batch ([B, z_dim]); default: sample_noise(batch_size or 128)."""
        self._require_gpu(z)
        if z is None:
            z = self.sample_noise(128 if batch_size is None else batch_size)
        z = _f32c(z).view(-1, self.z_dim)
        x = _GenFn.apply(self, z, *self.parameters())
        return x, self.loss(x)


# ---------------------------------------------------------------------------------------------------------------
# implicit-posterior VAE
# ---------------------------------------------------------------------------------------------------------------
def normal_energy_func(x, mu=0., logvar=0.):
    """utils/energy.py:74-77 (the only prior energy the HIP engine implements)."""
    x = x.view(x.size(0), -1)
    return torch.sum(0.5 * (logvar + (x - mu) ** 2 / math.exp(logvar) + math.log(2. * math.pi)), dim=1)


class _VaeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, noise, beta, nz, *params):
        d = mod._desc
        B = x.size(0)
        ws = mod._ws(L.query("ardae_model_workspace_floats", d, B, nz, 1))
        z = torch.empty(B * nz, mod.z_dim, device=x.device)
        losses = torch.empty(3, device=x.device)
        L.call("ardae_model_vae_forward", d, mod._flat, mod._packed_weights(), x, noise, B, nz, float(beta), ws, ws.numel(), z, losses)
        ctx.mod, ctx.ws, ctx.x, ctx.noise, ctx.beta, ctx.nz = mod, ws, x, noise, float(beta), nz
        ctx.mark_non_differentiable(losses)
        return z.view(B, nz, mod.z_dim), losses[0].clone(), losses

    @staticmethod
    def backward(ctx, dz, dloss, _dlosses):
        mod = ctx.mod
        B = ctx.x.size(0)
        grads = torch.empty_like(mod._flat)
        dl = float(dloss) if dloss is not None else 0.0
        dzc = _f32c(dz).view(B * ctx.nz, mod.z_dim) if dz is not None else None
        L.call("ardae_model_vae_backward", mod._desc, mod._flat, mod._packed_weights(), ctx.x, ctx.noise, B, ctx.nz, ctx.beta, dl, dzc, ctx.ws,
               ctx.ws.numel(), grads, 0.0)
        return (None,) * 5 + tuple(mod.param_views(grads))


def _weight_norm_init(spec, p):
    """WNlinear / WNconv2d / WeightNormalizedLinear.reset_parameters (layers2.py:66-71,184-190, layers.py:40-45) on the weight-normalised operators
    among the parameters p (under torch.no_grad()): direction and bias U(+-1/sqrt(in_features | in_channels)), scale 1."""
    for name, t in p.items():
        if name.endswith(".scale"):
            t.fill_(1.0)
        elif name.endswith(".direction") or (name[:-len("bias")] + "direction") in spec:
            d = spec[name if name.endswith(".direction") else name[:-len("bias")] + "direction"]
            t.uniform_(-1.0 / math.sqrt(d[1]), 1.0 / math.sqrt(d[1]))


class ImplicitPosteriorVAE(FlatParamModule):
    _kind = None
    _packed_floats_fn, _pack_fn = "ardae_model_packed_floats", "ardae_model_pack"
    _enc_types = ("concat",)
    return_samples = True        # forward() also returns the decoder sample / mean the reference's visualisation code reads

    def __init__(self, energy_func=normal_energy_func, input_dim=784, noise_dim=100, h_dim=300, z_dim=32, nonlinearity="softplus",
                 num_hidden_layers=1, init="gaussian", enc_type="concat"):
        super().__init__()
        assert enc_type in self._enc_types               # ivae/mnist.py:224; the other toy encoders are out of scope
        if energy_func is not normal_energy_func:
            raise NotImplementedError("only utils.normal_energy_func is implemented on the HIP path")
        if nonlinearity not in (("elu",) if self._kind in ("resconv", "auxresconv") else tuple(k for k in L.ACT if k not in ("none", None))):
            raise NotImplementedError(f"nonlinearity {nonlinearity!r}")
        self.energy_func = energy_func
        self.input_dim, self.noise_dim, self.h_dim, self.z_dim = input_dim, noise_dim, h_dim, z_dim
        self.latent_dim = z_dim
        self.nonlinearity, self.num_hidden_layers, self.init, self.enc_type = nonlinearity, num_hidden_layers, init, enc_type
        flags = L.MODEL_NO_CENTER if self._kind in ("resconv", "auxresconv") and not getattr(self, "do_center", True) else 0
        flags |= getattr(self, "_flag_extra", 0)
        self._desc = L.ModelDesc(KIND_IDS[self._kind], input_dim, noise_dim, h_dim, z_dim, num_hidden_layers, L.ACT[nonlinearity], flags)
        self._abi = (self._desc,)
        # floats per row of a sampler draw: the aux models take two draws per call, laid out side by side [eps0 | eps]
        self._noise_width = noise_dim + z_dim if self._kind in AUX_KINDS else noise_dim
        # columns of the `hidden1a` cDAE context (ivae_ardae.py:572-580): cat(h0, h) for the MLP / conv aux models, h alone for auxresconv
        self.hidden_dim = {"auxmnist": 2 * h_dim, "auxconv": 2 * h_dim, "auxresconv": h_dim, "auxtoy": 2 * h_dim}.get(self._kind, 0)
        self._build_params(layout.model_spec(self._kind, input_dim, noise_dim, h_dim, z_dim, num_hidden_layers, **getattr(self, "_spec_extra", {})),
                           {"encode": _EncodeBox})
        object.__setattr__(self.encode, "_owner_ref", weakref.ref(self))   # `model.encode(x, std=0)` (ivae_ardae.py:735)
        self.reset_parameters()

    def reset_parameters(self):
        self._default_init()
        with torch.no_grad():
            p = dict(self.named_parameters())
            if self._kind in ("resconv", "auxresconv"):
                _weight_norm_init(dict(self._spec), p)    # the plain nn.Linear layers of the aux sampler keep torch's default
                return
            if self._kind == "auxmnist":                  # self.apply(weight_init) on the whole model (ivae/auxmnist.py:172-174)
                if self.do_xavier:
                    for t in p.values():
                        nn.init.xavier_uniform_(t) if t.dim() == 2 else t.zero_()
                return
            if self._kind in ("conv", "auxconv"):         # self.apply(weight_init): xavier-uniform on Conv2d / Linear, zero biases;
                if self.do_xavier:                        # ConvTranspose2d keeps torch's default init (vae/auxconv.py:18-23)
                    for name, t in p.items():
                        if "deconv" in name or "logit_fn" in name:
                            continue
                        nn.init.xavier_uniform_(t) if t.dim() >= 2 else t.zero_()
                return
            if self._kind == "auxtoy":                    # init='gaussian' reaches the toy Decoder only (ivae/auxtoy.py:165, vae/toy.py)
                if self.init == "gaussian":
                    p["decode.reparam.mean_fn.weight"].normal_()
                return
            if self._kind == "mnist":                     # decode.apply(weight_init): xavier-uniform W, zero b (ivae/mnist.py:20-25,235)
                for name, t in p.items():
                    if name.startswith("decode."):
                        nn.init.xavier_uniform_(t) if t.dim() == 2 else t.zero_()
            else:                                         # ivae/toy.py:719-720
                if self.init == "gaussian":
                    p["decode.reparam.mean_fn.weight"].normal_()
            if self.init == "gaussian":                   # ivae/mnist.py:158-159
                p["encode.fc.fc.weight"].normal_()

    def _set_logvar_clips(self, clip_z0_logvar, clip_z_logvar):
        """clip_z0_logvar / clip_z_logvar of the hierarchical MLP models (ivae/auxmnist.py:144-161: 'none' -> None; the choices are
        NormalDistribution.clip_logvar's, models/reparam.py:17-41; any other name leaves the log-variance as it is there, and is refused here)."""
        for c in (clip_z0_logvar, clip_z_logvar):
            if c not in L.LOGVAR_CLIP:
                raise NotImplementedError(f"clip_logvar {c!r}: models/reparam.py:17-41 knows {sorted(k for k in L.LOGVAR_CLIP if k)}")
        self.clip_z0_logvar = None if clip_z0_logvar == "none" else clip_z0_logvar
        self.clip_z_logvar = None if clip_z_logvar == "none" else clip_z_logvar
        self._flag_extra = (L.LOGVAR_CLIP[clip_z0_logvar] << L.MODEL_CLIP_Z0_SHIFT) | (L.LOGVAR_CLIP[clip_z_logvar] << L.MODEL_CLIP_Z_SHIFT)

    def _x(self, input):
        self._require_gpu(input)
        return _f32c(input).view(input.size(0), self.input_dim)

    def _sample(self, x, nz, std, noise):
        """z = f(x, std*eps) without autograd (the reference loop detaches every use: ivae_ardae.py:735,748-750)."""
        B = x.size(0)
        if not (noise is None and std is not None and float(std) == 0.0):      # encode(x, std=0): the draw is multiplied by zero (NULL)
            if noise is None:
                noise = rng.normal((self._noise_numel(B, nz),), x.device)
                if std is not None:
                    noise = noise * float(std)
            noise = self._noise_rows(noise, B * nz)
        ws = self._ws(L.query("ardae_model_workspace_floats", self._desc, B, nz, 0))
        z = torch.empty(B * nz, self.z_dim, device=x.device)
        L.call("ardae_model_encode", self._desc, self._flat, self._packed_weights(), x, noise, B, nz, ws, ws.numel(), z)
        return z.view(B, nz, self.z_dim)

    def _noise_numel(self, B, nz):
        """Floats of one sampler call's draws for B images x nz rows."""
        return B * nz * self._noise_width

    def _noise_rows(self, noise, rows):
        """[rows, noise width] fp32 contiguous; the aux models also take the pair (eps0 [rows, noise_dim], eps [rows, z_dim])."""
        if isinstance(noise, (tuple, list)):
            noise = torch.cat([_f32c(n).view(rows, -1) for n in noise], 1)
        return _f32c(noise).view(rows, self._noise_width)

    def forward_hidden(self, input, std=None, nz=1, noise=None):
        return self._sample(self._x(input), nz, std, noise)

    def _hidden(self, input):
        """cat(h0, h) [B, 2 h] of the std = 0 pass (aux models; the `hidden1a` cDAE context)."""
        if self._kind not in AUX_KINDS:
            raise NotImplementedError("hidden contexts exist for the aux models only")
        x = self._x(input)
        B = x.size(0)
        ws = self._ws(L.query("ardae_model_workspace_floats", self._desc, B, 1, 0))
        hid = torch.empty(B, self.hidden_dim, device=x.device)
        L.call("ardae_model_encode_hidden", self._desc, self._flat, self._packed_weights(), x, B, ws, ws.numel(), None, hid)
        return hid

    def _decoder_sample(self, z_rows, dec_noise=None):
        """(x_sample, decoder mean) of the reference's Decoder.forward for z_rows [R, z]: Bernoulli decoders return the relaxed
        (logistic-sigmoid, T = 1) sample and sigmoid(logit) (reparam.py:111-158, ivae/mnist.py:188-199,300); the toy model's
        Gaussian decoder returns mu + exp(logvar/2) eps and mu (reparam.py:42-51, ivae/toy.py:725-737,858).  dec_noise injects
        the draw (uniform [R, D] resp. normal [R, D]); default: the library's Philox stream."""
        out = self.decode_params(z_rows)
        R = out[0].size(0)
        sample = torch.empty_like(out[0])
        if self._kind in GAUSSIAN_DECODERS:
            e = _f32c(dec_noise).view(R, self.input_dim) if dec_noise is not None else rng.normal((R, self.input_dim), out[0].device)
            L.call("ardae_gaussian_sample", out[0], out[1], e, out[0].numel(), sample)
            return sample, out[0]
        u = _f32c(dec_noise).view(R, self.input_dim) if dec_noise is not None else rng.uniform((R, self.input_dim), out[0].device)
        mean = torch.empty_like(out[0])
        L.call("ardae_relaxed_bernoulli", out[0], u, out[0].numel(), 1.0, sample, mean)
        return sample, mean

    def forward(self, input, beta=1.0, eta=0.0, lmbd=0.0, std=None, nz=1, noise=None, dec_noise=None):
        """-> (x_sample, decoder mean, z, loss, recon.detach(), prior.detach()) like the reference (ivae/mnist.py:267-301).
        The first two entries feed only the reference's visualisation code; they cost one extra decoder pass on the B*nz rows
        and are skipped (None, None) when `self.return_samples` is False - the fused engine never produces them."""
        if lmbd > 0:
            raise NotImplementedError                     # ivae/mnist.py:288-290
        x = self._x(input)
        B = x.size(0)
        if noise is None:
            noise = rng.normal((self._noise_numel(B, nz),), x.device)
            if std is not None:
                noise = noise * float(std)
        noise = self._noise_rows(noise, B * nz)
        z, loss, losses = _VaeFn.apply(self, x, noise, beta, nz, *self.parameters())
        xs, xm = (None, None)
        if self.return_samples:
            with torch.no_grad():
                xs, xm = self._decoder_sample(z.detach().reshape(B * nz, self.z_dim), dec_noise)
        return xs, xm, z, loss, losses[1].detach(), losses[2].detach()


    # ---- evaluation --------------------------------------------------------------------------------
    def decode_params(self, z):
        """Decoder heads for z [R, z_dim] -> (logits,) or (mean, logvar)."""
        self._require_gpu(z)
        z = _f32c(z).view(-1, self.z_dim)
        R = z.size(0)
        ws = self._ws(L.query("ardae_model_workspace_floats", self._desc, R, 1, 2))
        o0 = torch.empty(R, self.input_dim, device=z.device)
        o1 = torch.empty(R, self.input_dim, device=z.device) if self._kind in GAUSSIAN_DECODERS else None
        L.call("ardae_model_decode", self._desc, self._flat, self._packed_weights(), z, R, ws, ws.numel(), o0, o1)
        return (o0,) if o1 is None else (o0, o1)

    def generate(self, batch_size=1, z=None, dec_noise=None):
        """-> (x_sample, decoder mean, z) with z ~ N(0, I) (ivae/mnist.py:303-316, ivae/toy.py:862-873).  z / dec_noise inject the draws."""
        with torch.no_grad():
            z = rng.normal((batch_size, self.z_dim), self._flat.device) if z is None else _f32c(z).view(batch_size, self.z_dim)
            xs, xm = self._decoder_sample(z, dec_noise)
        return xs, xm, z

    def logprob(self, input, sample_size=128, z=None, std=None, enc_noise=None, prop_noise=None):
        """IWAE-k bound with a full-covariance Gaussian fitted to the encoder samples as proposal
        (logprob_w_cov_gaussian_posterior, ivae/mnist.py:378-437).  All images are processed at once: sampler and decoder
        are the HIP kernels, the k x z covariance / Cholesky / log-mean-exp glue is batched torch (off the timed path).
        enc_noise [B, k, noise_dim] (aux models: the pair ([B, k, noise_dim], [B, k, z])) / prop_noise [B, k, z] inject the draws."""
        x = self._x(input)
        B, k, zd = x.size(0), sample_size, self.z_dim
        assert sample_size >= 2 * self.z_dim                 # ivae/mnist.py:382
        with torch.no_grad():
            ke = k * k if self._kind == "auxtoy" else k       # ToyAuxIPVAE fits the proposal to Encoder._forward(nz=k): k z0's x k z's (ivae/auxtoy.py:313)
            if self._kind == "auxtoy":
                if enc_noise is not None and not isinstance(enc_noise, (tuple, list)):
                    raise ValueError("ToyAuxIPVAE.logprob: enc_noise is the pair (eps0 [B, k, noise_dim], eps [B, k k, z_dim])")
            elif isinstance(enc_noise, (tuple, list)):
                enc_noise = tuple(n.reshape(B * k, -1) for n in enc_noise)
            elif enc_noise is not None:
                enc_noise = enc_noise.reshape(B * k, self._noise_width)
            zs = self._sample(x, ke, std, enc_noise)          # [B,k,z]
            mu = zs.mean(1)
            zc = zs - mu.unsqueeze(1)
            cov = zc.transpose(1, 2) @ zc / (ke - 1)          # utils/stat.py:127-158
            if self._kind in AUX_KINDS:
                cov = cov + 1e-5 * torch.eye(zd, device=cov.device)      # ivae/auxmnist.py:321, ivae/auxconv.py, ivae/auxresconv.py:299
            cov = cov.contiguous()
            if zd <= 64:
                Lc = torch.empty_like(cov)                    # all B factorisations in one launch (MultivariateNormal's, ivae/mnist.py:397)
                L.call("ardae_cholesky_batched", cov, B, zd, Lc)
            else:
                # the LDS-resident kernel holds one z x z matrix per workgroup (z <= 64, every shipped recipe has z 32); larger latent
                # spaces factorise on the device through the library solver MultivariateNormal itself would use - evaluation only
                Lc, info = torch.linalg.cholesky_ex(cov)
                Lc = torch.where((info == 0).view(B, 1, 1), Lc, torch.full_like(Lc, float("nan")))
            if not bool(torch.isfinite(Lc).all()):
                raise ValueError("logprob: a sample covariance is not positive definite (torch.distributions would raise here too)")
            if prop_noise is None:
                prop_noise = rng.normal((B, k, zd), x.device)
            e = _f32c(prop_noise).view(B, k, zd)
            newz = (mu.unsqueeze(1) + e @ Lc.transpose(1, 2)).contiguous()
            logq = -0.5 * (e ** 2).sum(2) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1, keepdim=True) - 0.5 * zd * math.log(2 * math.pi)
            out = self.decode_params(newz.view(B * k, zd))
            rec = torch.empty(B * k, device=x.device); pri = torch.empty(B * k, device=x.device)
            L.call("ardae_model_loss_rows", self._desc, out[0], out[1] if len(out) > 1 else None, x, newz, B * k, k, rec, pri)
            lw = -rec.view(B, k) - pri.view(B, k) - logq
            m, _ = lw.max(1, keepdim=True)
            return (torch.log(torch.mean((lw - m).exp(), 1, keepdim=True) + 1e-10) + m).mean()


class MNISTIPVAE(ImplicitPosteriorVAE):
    """models/ivae/mnist.py::ImplicitPosteriorVAE (`--model mnist-concat`)."""
    _kind = "mnist"


class ConvIPVAE(ImplicitPosteriorVAE):
    """models/ivae/conv.py::ImplicitPosteriorVAE (`--model mnist-conv`, BASELINE config #4).  The reference's decoder only
    produces 28x28 outputs (cfg #5 note), so input_height=28 / input_channels=1 are required."""
    _kind = "conv"

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z_dim=32, noise_dim=100,
                 nonlinearity="softplus", do_xavier=True):
        if input_height != 28 or input_channels != 1:
            raise NotImplementedError("ConvIPVAE: the reference decoder (models/vae/conv.py:79-136) is hard-wired to 28x28x1")
        self.input_height, self.input_channels, self.do_xavier = input_height, input_channels, do_xavier
        super().__init__(energy_func, input_height * input_height * input_channels, noise_dim, 800, z_dim, nonlinearity, 1, "none", "concat")


class MNISTAuxIPVAE(ImplicitPosteriorVAE):
    """models/ivae/auxmnist.py::ImplicitPosteriorVAE (`--model auxmnist`, the shipped "hierarchical mlp" recipe): AuxEncoder -> z0 ->
    SimpleEncoder -> z, both Gaussian reparameterisations, `enc_type='simple'`; `clip_z0_logvar` / `clip_z_logvar`: the `clip_logvar` choices of
    models/reparam.py:17-41 ('hard', 'softplus', 'spm10' .. 'spm2', 'tanh', '2tanh'; 'none' in the shipped recipe).  A sampler call takes two draws;
    `noise=` accepts the pair (eps0 [rows, noise_dim], eps [rows, z_dim]) or one [rows, noise_dim + z_dim] tensor."""
    _kind = "auxmnist"
    _enc_types = ("simple",)

    def __init__(self, energy_func=normal_energy_func, input_dim=784, noise_dim=100, h_dim=300, z_dim=32, nonlinearity="softplus",
                 num_hidden_layers=2, enc_type="simple", clip_z0_logvar=None, clip_z_logvar=None, do_xavier=True):
        if enc_type != "simple":
            raise NotImplementedError                     # ivae/auxmnist.py:72-73
        self.do_xavier = do_xavier
        self._set_logvar_clips(clip_z0_logvar, clip_z_logvar)
        super().__init__(energy_func, input_dim, noise_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, "none", enc_type)


class ToyAuxIPVAE(ImplicitPosteriorVAE):
    """models/ivae/auxtoy.py::ImplicitPosteriorVAE (`--model auxmlp`, ivae_ardae.py:443-454): MNISTAuxIPVAE's networks without the 2x - 1 rescale,
    the toy problem's Gaussian decoder, and a SQUARE sampling scheme - a call with nz rows per image draws q = int(sqrt(nz)) z0's per image and
    q z's per z0 (`forward_hidden` / `forward`, :215,230; nz must be a square), `logprob(sample_size=k)` fits its proposal to k x k encoder
    samples (:313).  `noise=` of a sampler call: the pair (eps0 [B q, noise_dim], eps [B q q, z_dim]) or ONE flat tensor [eps0 block | eps block]."""
    _kind = "auxtoy"
    _enc_types = ("simple",)

    def __init__(self, energy_func=normal_energy_func, input_dim=2, noise_dim=2, h_dim=64, z_dim=2, nonlinearity="tanh", num_hidden_layers=1,
                 init="gaussian", enc_type="simple", clip_z0_logvar=None, clip_z_logvar=None):
        if enc_type != "simple":
            raise NotImplementedError                     # ivae/auxtoy.py:70-71
        self._set_logvar_clips(clip_z0_logvar, clip_z_logvar)
        super().__init__(energy_func, input_dim, noise_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, init, enc_type)

    @staticmethod
    def _q(nz):
        q = math.isqrt(int(nz))
        if q * q != nz:
            raise ValueError(f"ToyAuxIPVAE draws q z0's x q z's per image: nz = {nz} is not a square (ivae/auxtoy.py:215)")
        return q

    def _noise_numel(self, B, nz):
        return B * self._q(nz) * self.noise_dim + B * nz * self.z_dim

    def _noise_rows(self, noise, rows):
        if isinstance(noise, (tuple, list)):
            noise = torch.cat([_f32c(n).reshape(-1) for n in noise])
        return _f32c(noise).reshape(-1)


class MNISTConvAuxIPVAE(ImplicitPosteriorVAE):
    """models/ivae/auxconv.py::ImplicitPosteriorVAE (`--model auxconv`, the shipped "hierarchical conv" recipe): the hierarchical
    sampler with two conv trunks and ConvIPVAE's decoder; 28x28x1 only; the hidden1a context is [B, 1600]."""
    _kind = "auxconv"

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z0_dim=100, h_dim=300, z_dim=32,
                 nonlinearity="softplus", do_xavier=True):
        if input_height != 28 or input_channels != 1:
            raise NotImplementedError("MNISTConvAuxIPVAE: the reference decoder (models/vae/conv.py:79-136) is hard-wired to 28x28x1")
        self.input_height, self.input_channels, self.z0_dim, self.do_xavier = input_height, input_channels, z0_dim, do_xavier
        super().__init__(energy_func, 784, z0_dim, 800, z_dim, nonlinearity, 1, "none", "concat")


class ResConvIPVAE(ImplicitPosteriorVAE):
    """models/ivae/resconv.py::ImplicitPosteriorVAE as the ten `--model resconv*` choices build it (ivae_ardae.py:323-442): weight-normalised
    residual-conv trunk and decoder, ELU, 28x28x1, c_dim 512, do_center either way, and every sampler head of `enc_type`:
    'mlp' (resconv / resconvct), 'res-wn-mlp' (-res: the shipped "implicit resconv" recipe), 'res-mlp' (-res2), 'res-wn-mlp-lin' (-res3),
    'res-mlp-lin' (-res4), with 1 .. 4 hidden layers (`--model-n-layers`)."""
    _kind = "resconv"

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z_dim=32, noise_dim=100, c_dim=512, h_dim=800,
                 num_hidden_layers=1, nonlinearity="elu", do_center=False, do_m5bias=False, enc_noise=False, enc_type="mlp"):
        if input_height != 28 or input_channels != 1:
            raise AssertionError("input_height == 28 and input_channels == 1")           # ivae/resconv.py:218-219
        assert enc_type in layout.RESCONV_HEADS                                          # ivae/resconv.py:77
        assert num_hidden_layers > 0                                                     # ivae/resconv.py:73
        if enc_noise or do_m5bias or c_dim != 512 or num_hidden_layers > 4:
            raise NotImplementedError("the HIP engine builds ResConvIPVAE as ivae_ardae.py's --model resconv* choices do: c_dim=512, no enc_noise / "
                                      "do_m5bias, at most 4 hidden layers (any enc_type, do_center either way)")
        if enc_type != "mlp" and c_dim + noise_dim == h_dim:
            raise NotImplementedError("c_dim + noise_dim == h_dim makes the first ResLinear's skip the concatenated input itself; not built")
        self._flag_extra = layout.RESCONV_HEADS[enc_type] << L.MODEL_HEAD_SHIFT
        self._spec_extra = {"enc_type": enc_type}
        self.input_height, self.input_channels, self.c_dim = input_height, input_channels, c_dim
        self.do_center, self.do_m5bias, self.enc_noise = do_center, do_m5bias, enc_noise
        super().__init__(energy_func, 784, noise_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, "none", "concat")
        self.enc_type = enc_type


class MNISTResConvAuxIPVAE(ImplicitPosteriorVAE):
    """models/ivae/auxresconv.py::ImplicitPosteriorVAE (`--model auxresconvct`, the shipped "hierarchical resconv" recipe): the
    residual-conv trunk shared by a Gaussian z0 head and the z head (log-variances clipped 'spm4'), the residual-conv decoder; its
    hidden1a cDAE context is h [B, c_dim].  A sampler call takes two draws: noise = (eps0 [rows, z0_dim], eps [rows, z_dim])."""
    _kind = "auxresconv"

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z0_dim=100, z_dim=32, c_dim=450, nonlinearity="elu",
                 do_center=False, do_m5bias=False):
        assert input_height == 28 and input_channels == 1 and nonlinearity == "elu"     # ivae/auxresconv.py:67-69
        if do_m5bias:
            raise NotImplementedError("the HIP engine builds MNISTResConvAuxIPVAE as --model auxresconvct / auxresconv do (no do_m5bias; do_center either way)")
        self.input_height, self.input_channels, self.z0_dim, self.c_dim, self.do_center, self.do_m5bias = input_height, input_channels, z0_dim, c_dim, bool(do_center), False
        super().__init__(energy_func, 784, z0_dim, c_dim, z_dim, nonlinearity, 1, "none", "concat")


class MNISTResConvAuxIPVAEClipped(MNISTResConvAuxIPVAE):
    """models/ivae/auxresconv2.py::ImplicitPosteriorVAE (`--model auxresconv-clip` / `auxresconvct-clip`, ivae_ardae.py:507-534): the
    same networks with the two log-variance heads built WITHOUT the 'spm4' clip (:71-72) and z0 = mu0 + (std exp(lv0 / 2) + 1) eps0
    (`sample_gaussian(..., min_std=1.)`, :29-36,91).  Consequence the training loop inherits: `encode(x, std=0)` /
    `forward_hidden(x, std=0)` are RANDOM draws here (z0 = mu0 + eps0).  `noise` of a std = 0 call is that unscaled eps0 [B, z0_dim]
    (default: a fresh Philox draw); other calls take unscaled draws (std None / 1: the only values the reference's loop uses)."""
    _clipped = True

    def __init__(self, *a, **k):
        self._flag_extra = L.MODEL_CLIPPED
        super().__init__(*a, **k)

    def _std0(self, x, raw0, want_hidden):
        B = x.size(0)
        raw = _f32c(raw0).view(B, -1)[:, :self.z0_dim].contiguous() if raw0 is not None else rng.normal((B, self.z0_dim), x.device)
        ws = self._ws(L.query("ardae_model_workspace_floats", self._desc, B, 1, 0))
        out = torch.empty(B, self.hidden_dim if want_hidden else self.z_dim, device=x.device)
        L.call("ardae_model_encode_hidden_raw", self._desc, self._flat, self._packed_weights(), x, raw, B, ws, ws.numel(),
               None if want_hidden else out, out if want_hidden else None)
        return out

    def _sample(self, x, nz, std, noise):
        if std is not None and float(std) == 0.0:
            if nz != 1:
                raise NotImplementedError("the clipped class at std = 0 is built for nz = 1 (what ivae_ardae.py:735-748,815-826 calls)")
            if isinstance(noise, (tuple, list)):
                noise = noise[0]
            return self._std0(x, noise, False).view(x.size(0), 1, self.z_dim)
        if std is not None and float(std) != 1.0:
            raise NotImplementedError("MNISTResConvAuxIPVAEClipped: std must be None, 1 or 0 (the unscaled eps0 term needs the draw and std apart)")
        return super()._sample(x, nz, None, noise)

    def _hidden(self, input, raw0=None):
        return self._std0(self._x(input), raw0, True)


class ToyIPVAE(ImplicitPosteriorVAE):
    """models/ivae/toy.py::ImplicitPosteriorVAE with enc_type='concat' (`--model mlp-concat`)."""
    _kind = "toy"

    def __init__(self, energy_func=normal_energy_func, input_dim=2, noise_dim=2, h_dim=64, z_dim=2, nonlinearity="tanh",
                 num_hidden_layers=1, init="gaussian", enc_type="scale"):
        if enc_type != "concat":
            raise NotImplementedError(f"enc_type {enc_type!r}: only 'concat' is on the BASELINE path (SURVEY 2 #5)")
        super().__init__(energy_func, input_dim, noise_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, init, enc_type)


# ---------------------------------------------------------------------------------------------------------------
# Gaussian-posterior VAE baselines (vae.py)
# ---------------------------------------------------------------------------------------------------------------
class _GaussVaeFn(torch.autograd.Function):
    """VAE.forward through ardae_vae_forward; backward = ardae_vae_backward with the incoming d loss as loss_scale (the workspace keeps
    the activations).  Only `loss` carries a gradient: z, mu and logvar are returned detached, as nothing in vae.py differentiates them."""

    @staticmethod
    def forward(ctx, mod, x, eps, beta, *params):
        d, B = mod._desc, x.size(0)
        ws = mod._ws(L.query("ardae_model_workspace_floats", d, B, 1, 1))
        z, eps_out = torch.empty(B, mod.z_dim, device=x.device), torch.empty(B, mod._eps_width, device=x.device)
        losses = torch.empty(3, device=x.device)
        seed, offset = rng.get_state()["seed"], (rng._next_offset() if eps is None else 0)
        L.call("ardae_vae_forward", d, mod._flat, mod._packed_weights(), x, eps, B, float(beta), 1.0, seed, offset, None, ws, ws.numel(), z, eps_out,
               losses)
        ctx.mod, ctx.ws, ctx.x, ctx.beta = mod, ws, x, float(beta)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(z, eps_out, losses)
        return losses[0].clone(), z, eps_out, losses

    @staticmethod
    def backward(ctx, dloss, *_unused):
        mod = ctx.mod
        grads = torch.empty_like(mod._flat)
        L.call("ardae_vae_backward", mod._desc, mod._flat, mod._packed_weights(), ctx.x, ctx.x.size(0), ctx.beta, 0.0 if dloss is None else float(dloss),
               ctx.ws, ctx.ws.numel(), grads, 0.0)
        return (None,) * 4 + tuple(mod.param_views(grads))


class _GaussEncodeBox(_Box):
    """`model.encode(x)` -> (z, mu, logvar) like Encoder.forward (vae/mnist.py:49-63), without autograd; `eps` injects the draw."""

    def forward(self, x, eps=None):
        o = self._owner_ref()
        mu, lv = o.encode_stats(x)
        e = rng.normal(tuple(mu.shape), mu.device) if eps is None else _f32c(eps).view_as(mu)
        z = torch.empty_like(mu)
        L.call("ardae_gaussian_sample", mu, lv, e, mu.numel(), z)
        return z, mu, lv

    def sample(self, mu, logvar, eps=None):
        """NormalDistributionLinear.sample_gaussian (models/reparam.py:42-51)."""
        e = rng.normal(tuple(mu.shape), mu.device) if eps is None else _f32c(eps).view_as(mu)
        z = torch.empty_like(mu)
        L.call("ardae_gaussian_sample", _f32c(mu), _f32c(logvar), e, mu.numel(), z)
        return z


class GaussianVAE(FlatParamModule):
    """What MNISTVAE, ToyVAE, MNISTConvVAE and MNISTResConvVAE share: ardae_model_desc kinds 8 / 9 / 11 / 12, an encoder with a Gaussian head and its analytic KL, the
    decoders of the implicit models.  A family is its `_kind` and its `_param_spec()`.  There is no CPU path."""
    _kind = None                 # "vae_mnist" | "vae_toy" | "vae_conv" | "vae_resconv"
    _packed_floats_fn, _pack_fn = "ardae_model_packed_floats", "ardae_model_pack"
    return_samples = True        # forward() also returns the decoder sample / mean (one extra decoder pass); False: (None, None)
    noise_dim = 0
    _eps_width = property(lambda self: self.z_dim)      # floats per image of forward()'s draw (the auxiliary-variable models: noise_dim + z_dim)
    _eval_groups = None          # GaussianIwaeEvaluator: (images per encoder / ELBO-decoder call, images per importance-sample decoder call); None: a chunk at once

    def _build(self, energy_func, input_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, flags=0, noise_dim=0, boxes=None):
        if energy_func is not normal_energy_func:
            raise NotImplementedError("only utils.normal_energy_func is implemented on the HIP path")
        if nonlinearity not in L.ACT or nonlinearity in ("none", None):
            raise NotImplementedError(f"nonlinearity {nonlinearity!r}")
        if not (int(input_dim) >= 1 and int(h_dim) >= 1 and int(z_dim) >= 1 and 1 <= int(num_hidden_layers) <= 4):
            raise ValueError(f"{type(self).__name__}: dimensions must be positive and 1 <= num_hidden_layers <= 4 (got input_dim={input_dim}, "
                             f"h_dim={h_dim}, z_dim={z_dim}, num_hidden_layers={num_hidden_layers})")
        self.energy_func = energy_func
        self.input_dim, self.h_dim, self.z_dim = int(input_dim), int(h_dim), int(z_dim)
        self.latent_dim = self.z_dim
        self.nonlinearity, self.num_hidden_layers = nonlinearity, int(num_hidden_layers)
        self._desc = L.ModelDesc(KIND_IDS[self._kind], self.input_dim, int(noise_dim), self.h_dim, self.z_dim, self.num_hidden_layers, L.ACT[nonlinearity], flags)
        self._abi = (self._desc,)
        self._build_params(self._param_spec(), {"encode": _GaussEncodeBox} if boxes is None else boxes)
        object.__setattr__(self.encode, "_owner_ref", weakref.ref(self))
        self.reset_parameters()

    def _param_spec(self):
        """Names and shapes in named_parameters() order (the two MLP families; the conv families have their own)."""
        return layout.vae_spec(self._kind[len("vae_"):], self.input_dim, self.h_dim, self.z_dim, self.num_hidden_layers)

    _x = ImplicitPosteriorVAE._x
    decode_params = ImplicitPosteriorVAE.decode_params
    _decoder_sample = ImplicitPosteriorVAE._decoder_sample

    def generate(self, batch_size=1, z=None, dec_noise=None):
        """-> (x_sample, decoder mean, z) with z ~ N(0, I) (vae/mnist.py:164-177, vae/toy.py:154-167).  z / dec_noise inject the draws."""
        self._require_gpu(z, dec_noise)
        return ImplicitPosteriorVAE.generate(self, batch_size, z, dec_noise)

    def encode_stats(self, input):
        """(mu, logvar) [B, z_dim] of q(z | x), no draw (ardae_vae_encode_stats)."""
        x = self._x(input)
        B = x.size(0)
        ws = self._ws(L.query("ardae_model_workspace_floats", self._desc, B, 1, 0))
        mu, lv = torch.empty(B, self.z_dim, device=x.device), torch.empty(B, self.z_dim, device=x.device)
        L.call("ardae_vae_encode_stats", self._desc, self._flat, self._packed_weights(), x, B, ws, ws.numel(), mu, lv)
        return mu, lv

    def forward(self, input, beta=1.0, eps=None, dec_noise=None):
        """-> (x_sample, decoder mean, z, loss, recon.detach(), kld.detach()) like the reference (vae/mnist.py:142-162).  `eps` [B, z_dim]
        injects the posterior draw (default: drawn in the head kernel from the library's host Philox stream), `dec_noise` the decoder's."""
        x = self._x(input)
        B = x.size(0)
        if eps is not None:
            self._require_gpu(eps)
            eps = _f32c(eps).view(B, self._eps_width)
        loss, z, _, losses = _GaussVaeFn.apply(self, x, eps, beta, *self.parameters())
        xs, xm = (None, None)
        if self.return_samples:
            with torch.no_grad():
                xs, xm = self._decoder_sample(z, dec_noise)
        return xs, xm, z, loss, losses[1].detach(), losses[2].detach()

    def logprob_rows(self, input, sample_size=128, eps=None):
        """The IWAE-`sample_size` bound of every image under the analytic posterior, [B] on the device (VAE.logprob before its mean,
        vae/mnist.py:179-217): encoder statistics, ardae_vae_iwae_draw (samples and log q in one launch), decoder, row losses,
        log-mean-exp.  eps [B, sample_size, z_dim] injects the draws."""
        x = self._x(input)
        B, k, zd = x.size(0), int(sample_size), self.z_dim
        if zd > 64:
            raise NotImplementedError(f"{type(self).__name__}.logprob: z_dim {zd} > 64: ardae_vae_iwae_draw takes latent widths up to 64")
        with torch.no_grad():
            mu, lv = self.encode_stats(x)
            if eps is not None:
                self._require_gpu(eps)
                eps = _f32c(eps).view(B, k, zd)
            z, logq = torch.empty(B * k, zd, device=x.device), torch.empty(B * k, device=x.device)
            L.call("ardae_vae_iwae_draw", mu, lv, eps, B, k, zd, rng.get_state()["seed"], rng._next_offset() if eps is None else 0, 0, z, logq, None)
            out = self.decode_params(z)
            rec, pri, res = torch.empty(B * k, device=x.device), torch.empty(B * k, device=x.device), torch.empty(B, device=x.device)
            L.call("ardae_model_loss_rows", self._desc, out[0], out[1] if len(out) > 1 else None, x, z, B * k, k, rec, pri)
            L.call("ardae_iwae_reduce", rec, pri, logq, B, k, res)
        return res

    def logprob(self, input, sample_size=128, z=None, eps=None):
        """VAE.logprob (vae/mnist.py:179-220; the reference ignores `z` too)."""
        return self.logprob_rows(input, sample_size, eps).mean()


class MNISTVAE(GaussianVAE):
    """models/vae/mnist.py::VAE (`vae.py --model mnist`, the "# mlp" baseline of run_vae_dbmnist.sh): x -> 2x - 1 inside the encoder, Bernoulli decoder."""
    _kind = "vae_mnist"

    def __init__(self, energy_func=normal_energy_func, input_dim=784, h_dim=300, z_dim=32, nonlinearity="softplus", num_hidden_layers=2,
                 do_xavier=False, do_m5bias=False):
        super().__init__()
        self.do_xavier, self.do_m5bias = do_xavier, do_m5bias
        self._build(energy_func, input_dim, h_dim, z_dim, nonlinearity, num_hidden_layers)

    def reset_parameters(self):
        self._default_init()
        with torch.no_grad():
            p = dict(self.named_parameters())
            if self.do_xavier:                              # self.apply(weight_init): xavier-uniform W, zero b (vae/mnist.py:16-21,125-127)
                for t in p.values():
                    nn.init.xavier_uniform_(t) if t.dim() == 2 else t.zero_()
            if self.do_m5bias:                              # vae/mnist.py:128-129
                p["decode.reparam.logit_fn.bias"].fill_(-5.0)


class MNISTConvVAE(GaussianVAE):
    """models/vae/conv.py::VAE (`vae.py --model conv`, the "# conv" baseline of run_vae_dbmnist.sh): ConvIPVAE's trunk, `encode.fc` 512 -> 800 and a
    Gaussian head; that model's decoder.  The reference's decoder only produces 28x28 outputs, so input_height=28 / input_channels=1 are required.
    forward() takes x as [B, 784] or [B, 1, 28, 28] and returns the decoder sample / mean as [B, 784]."""
    _kind = "vae_conv"
    # Every (transposed) convolution here is a linear on rows = images x positions, and the library picks a linear's kernel by its row count;
    # the kernels add in different orders, so a row's last bits depend on the images per call - in the trunk and `fc` as in the decoder.  The
    # evaluator therefore calls the encoder and the ELBO pass's decoder on 64 images and the importance samples' decoder on 16 (at k = 256:
    # 4096 decoded rows, 0.2 G floats of workspace), and cuts its chunks at multiples of 64: what it reports does not depend on the budget.
    _eval_groups = (64, 16)

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z_dim=32, nonlinearity="softplus", do_xavier=False,
                 do_m5bias=False):
        if input_height != 28 or input_channels != 1:
            raise NotImplementedError("MNISTConvVAE: the reference decoder (models/vae/conv.py:79-136) is hard-wired to 28x28x1")
        super().__init__()
        self.input_height, self.input_channels, self.do_xavier, self.do_m5bias = input_height, input_channels, do_xavier, do_m5bias
        self._build(energy_func, input_height * input_height * input_channels, 800, z_dim, nonlinearity, 1)

    def _param_spec(self):
        return layout.conv_vae_spec(self.z_dim)

    def reset_parameters(self):
        self._default_init()
        with torch.no_grad():
            p = dict(self.named_parameters())
            if self.do_xavier:                              # self.apply(weight_init): xavier-uniform on Conv2d / Linear, zero biases; ConvTranspose2d
                for name, t in p.items():                   # keeps torch's default init (vae/conv.py:17-22,164-166)
                    if "deconv" in name or "logit_fn" in name:
                        continue
                    nn.init.xavier_uniform_(t) if t.dim() >= 2 else t.zero_()
            if self.do_m5bias:                              # vae/conv.py:167-168
                p["decode.reparam.logit_fn.bias"].fill_(-5.0)


class MNISTResConvVAE(GaussianVAE):
    """models/vae/resconv.py::VAE (`vae.py --model resconv`, the "# resconv" baseline of run_vae_sbmnist.sh): the weight-normalised residual-conv trunk
    of MNISTResConvAuxIPVAE (width c_dim) with a plain Gaussian head, and that model's decoder.  ELU only (vae/resconv.py:145), 28x28x1 only.
    do_center=True feeds the trunk 2x - 1; vae.py builds `resconv` and `resconvct` alike with do_center=False (vae.py:171-193).
    forward() takes x as [B, 784] or [B, 1, 28, 28] and returns the decoder sample / mean as [B, 784]."""
    _kind = "vae_resconv"
    # As for MNISTConvVAE every 3x3 convolution but the last stage is a linear on rows = images x positions whose kernel the library picks by the
    # row count, so the evaluator runs fixed groups: the encoder and the ELBO pass's decoder on 64 images per call, the importance samples' decoder on
    # 8.  The decode-only workspace of this kind (one columns scratch, the last stage fused) takes ~1.18e5 floats per decoded row against ~3.5e5 for
    # the training carving: at k = 256 the 2048 rows of a call need 0.24 G floats, inside the default budget of 2^28; the training carving would
    # allow 2 images.  Chunks are cut at multiples of 64.
    _eval_groups = (64, 8)

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z_dim=32, c_dim=450, nonlinearity="elu", do_center=False,
                 do_m5bias=False):
        if input_height != 28 or input_channels != 1:
            raise NotImplementedError("MNISTResConvVAE: the reference asserts 28x28x1 (models/vae/resconv.py:143-144)")
        if nonlinearity != "elu":
            raise NotImplementedError(f"MNISTResConvVAE: nonlinearity {nonlinearity!r}: the reference asserts 'elu' (models/vae/resconv.py:145)")
        super().__init__()
        self.input_height, self.input_channels, self.c_dim = input_height, input_channels, int(c_dim)
        self.do_center, self.do_m5bias = bool(do_center), do_m5bias
        self._build(energy_func, input_height * input_height * input_channels, c_dim, z_dim, nonlinearity, 1, 0 if do_center else L.MODEL_NO_CENTER)

    def _param_spec(self):
        return layout.resconv_vae_spec(self.z_dim, self.c_dim)

    def reset_parameters(self):
        self._default_init()                                # the two heads: nn.Linear's default
        with torch.no_grad():
            p = dict(self.named_parameters())
            _weight_norm_init(dict(self._spec), p)
            if self.do_m5bias:                              # vae/resconv.py:107-108
                p["decode.dec.17.conv_01.bias"].normal_(-3.0, 0.0001)


class ToyVAE(GaussianVAE):
    """models/vae/toy.py::VAE (`vae.py --model toy`): no rescale, Gaussian decoder (decode.reparam.{mean_fn, logvar_fn})."""
    _kind = "vae_toy"

    def __init__(self, energy_func=normal_energy_func, input_dim=2, h_dim=64, z_dim=2, nonlinearity="softplus", num_hidden_layers=1, init="gaussian"):
        super().__init__()
        self.init = init
        self._build(energy_func, input_dim, h_dim, z_dim, nonlinearity, num_hidden_layers)

    def reset_parameters(self):
        self._default_init()
        if self.init == "gaussian":                         # Decoder.reset_parameters (vae/toy.py:75-81)
            with torch.no_grad():
                dict(self.named_parameters())["decode.reparam.mean_fn.weight"].normal_()


class _AuxGaussianVAE(GaussianVAE):
    """What MNISTAuxVAE, ToyAuxVAE, MNISTConvAuxVAE and MNISTResConvAuxVAE share (ardae_model_desc kinds 14 / 15 / 17 / 19): q(z0 | x) q(z | z0, x) with an auxiliary decoder r(z0 | z, x).  forward()'s
    `eps` is [B, noise_dim + z_dim], rows [eps0 | eps]; encode_stats() returns the statistics of q(z0 | x); logprob's `eps` is
    [B, sample_size, noise_dim + z_dim].  `model.encode` / `model.aux_encode` / `model.aux_decode` only name parameters: the three networks run inside
    forward() and logprob()."""
    _eps_width = property(lambda self: self.noise_dim + self.z_dim)

    def _build_aux(self, energy_func, input_dim, noise_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, enc_type, clip_logvar):
        if enc_type != "simple":
            raise NotImplementedError(f"enc_type {enc_type!r}: the reference builds 'simple' only (models/vae/auxmnist.py:294-302)")
        if clip_logvar not in L.LOGVAR_CLIP:
            raise NotImplementedError(f"clip_logvar {clip_logvar!r}: models/reparam.py:17-41 knows {sorted(k for k in L.LOGVAR_CLIP if k)}")
        if not 1 <= int(noise_dim) <= 128:
            raise ValueError(f"{type(self).__name__}: noise_dim must be 1 .. 128 (got {noise_dim})")
        self.noise_dim, self.enc_type = int(noise_dim), enc_type
        self.clip_logvar = None if clip_logvar == "none" else clip_logvar                       # vae/auxmnist.py:291
        self._build(energy_func, input_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, L.LOGVAR_CLIP[clip_logvar] << L.MODEL_CLIP_Z0_SHIFT,
                    noise_dim=self.noise_dim, boxes={})

    def _param_spec(self):
        return layout.aux_vae_spec(self._kind[len("vae_aux"):], self.input_dim, self.noise_dim, self.h_dim, self.z_dim, self.num_hidden_layers)

    def encode_stats(self, input):
        """(mu0, logvar0) [B, noise_dim] of q(z0 | x), the log-variance clipped, no draw (ardae_vae_encode_stats)."""
        x = self._x(input)
        B = x.size(0)
        ws = self._ws(L.query("ardae_model_workspace_floats", self._desc, B, 1, 0))
        mu, lv = torch.empty(B, self.noise_dim, device=x.device), torch.empty(B, self.noise_dim, device=x.device)
        L.call("ardae_vae_encode_stats", self._desc, self._flat, self._packed_weights(), x, B, ws, ws.numel(), mu, lv)
        return mu, lv

    def logprob_rows(self, input, sample_size=128, eps=None):
        """The IWAE-`sample_size` bound of every image, [B] on the device (VAE.logprob before its mean, vae/auxmnist.py:381-451 with
        sample_size2 = 1): the statistics of q(z0 | x), ardae_vae_aux_iwae_draw (k z0's, one z per z0, and log q(z0|x) + log q(z|z0,x) - log r(z0|z,x)
        as one row), decoder, row losses, log-mean-exp.  eps [B, sample_size, noise_dim + z_dim] injects the draws."""
        x = self._x(input)
        B, k, zd = x.size(0), int(sample_size), self.z_dim
        if zd > 128:
            raise NotImplementedError(f"{type(self).__name__}.logprob: z_dim {zd} > 128: ardae_vae_aux_iwae_draw takes latent widths up to 128")
        with torch.no_grad():
            mu0, lv0 = self.encode_stats(x)
            if eps is not None:
                self._require_gpu(eps)
                eps = _f32c(eps).view(B, k, self._eps_width)
            z, logq = torch.empty(B * k, zd, device=x.device), torch.empty(B * k, device=x.device)
            ws = self._ws(L.query("ardae_model_workspace_floats", self._desc, B, k, 4))
            seed = rng.get_state()["seed"]
            off0, off1 = (rng._next_offset(), rng._next_offset()) if eps is None else (0, 0)
            L.call("ardae_vae_aux_iwae_draw", self._desc, self._flat, self._packed_weights(), x, mu0, lv0, eps, B, k, seed, off0, off1, 0, ws, ws.numel(),
                   z, logq, None)
            out = self.decode_params(z)
            rec, pri, res = torch.empty(B * k, device=x.device), torch.empty(B * k, device=x.device), torch.empty(B, device=x.device)
            L.call("ardae_model_loss_rows", self._desc, out[0], out[1] if len(out) > 1 else None, x, z, B * k, k, rec, pri)
            L.call("ardae_iwae_reduce", rec, pri, logq, B, k, res)
        return res


class MNISTAuxVAE(_AuxGaussianVAE):
    """models/vae/auxmnist.py::VAE (`vae.py --model auxmnist`, the "# hierarchical mlp" baseline of run_vae_dbmnist.sh): the Gaussian counterpart of
    MNISTAuxIPVAE.  x -> 2x - 1 inside the three encoders, Bernoulli decoder; `clip_logvar` is aux_encode's."""
    _kind = "vae_auxmnist"

    def __init__(self, energy_func=normal_energy_func, input_dim=784, noise_dim=100, h_dim=300, z_dim=32, nonlinearity="softplus", num_hidden_layers=2,
                 enc_type="simple", clip_logvar=None, do_xavier=True, do_m5bias=False):
        super().__init__()
        self.do_xavier, self.do_m5bias = do_xavier, do_m5bias
        self._build_aux(energy_func, input_dim, noise_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, enc_type, clip_logvar)

    reset_parameters = MNISTVAE.reset_parameters        # weight_init where do_xavier, the -5 logit bias where do_m5bias (vae/auxmnist.py:307-311)


class ToyAuxVAE(_AuxGaussianVAE):
    """models/vae/auxtoy.py::VAE (`vae.py --model auxtoy`): the same networks without the rescale, the Gaussian decoder of models/vae/toy.py."""
    _kind = "vae_auxtoy"

    def __init__(self, energy_func=normal_energy_func, input_dim=2, noise_dim=2, h_dim=64, z_dim=2, nonlinearity="tanh", num_hidden_layers=1,
                 init="gaussian", enc_type="simple", clip_logvar=None):
        super().__init__()
        self.init = init
        self._build_aux(energy_func, input_dim, noise_dim, h_dim, z_dim, nonlinearity, num_hidden_layers, enc_type, clip_logvar)

    reset_parameters = ToyVAE.reset_parameters          # Decoder.reset_parameters (vae/toy.py:75-81)


class MNISTConvAuxVAE(_AuxGaussianVAE):
    """models/vae/auxconv.py::VAE (`vae.py --model auxconv`, the "# hierarchical conv" baseline of run_vae_dbmnist.sh): the Gaussian counterpart of
    MNISTConvAuxIPVAE.  Three conv trunks on 2x - 1 (aux_encode, encode, aux_decode), each followed by an `fc` to 800 and a Gaussian head; z0 has width
    z0_dim (`noise_dim`), there is no log-variance clip; MNISTConvVAE's decoder.  28x28x1 only.  forward() takes x as [B, 784] or [B, 1, 28, 28] and
    returns the decoder sample / mean as [B, 784]."""
    _kind = "vae_auxconv"
    # As for MNISTConvVAE the library picks the kernel of every conv-as-linear (and of the stage linears) by the row count, so the evaluator runs fixed
    # groups: the statistics and the ELBO pass on 64 images per call, the three stages and the importance samples' decoder on 32.  The decode-only
    # workspace of this kind (the last two stages fused: no c2 / u2 / c3) takes ~1.62e4 floats per decoded row against ~5.18e4 for MNISTConvVAE's: at
    # k = 256 the 8192 rows of a call need 0.13 G floats, inside the default budget of 2^28 (64 images would need 0.27 G).  Chunks are cut at multiples
    # of 64 images.
    _eval_groups = (64, 32)

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z0_dim=100, z_dim=32, nonlinearity="softplus", do_xavier=True,
                 do_m5bias=False):
        if input_height != 28 or input_channels != 1:
            raise NotImplementedError("MNISTConvAuxVAE: the reference decoder (models/vae/conv.py:79-136) is hard-wired to 28x28x1")
        super().__init__()
        self.input_height, self.input_channels, self.do_xavier, self.do_m5bias = input_height, input_channels, do_xavier, do_m5bias
        self.z0_dim = int(z0_dim)
        self._build_aux(energy_func, input_height * input_height * input_channels, z0_dim, 800, z_dim, nonlinearity, 1, "simple", None)

    def _param_spec(self):
        return layout.aux_conv_vae_spec(self.noise_dim, self.z_dim)

    reset_parameters = MNISTConvVAE.reset_parameters    # weight_init on Conv2d / Linear where do_xavier (ConvTranspose2d keeps torch's init), the -5 logit bias where do_m5bias (vae/auxconv.py:18-23,231-235)


class MNISTResConvAuxVAE(_AuxGaussianVAE):
    """models/vae/auxresconv.py::VAE (`vae.py --model auxresconv` / `auxresconvct`): the Gaussian counterpart of MNISTResConvAuxIPVAE.  ONE
    weight-normalised residual-conv trunk `inp_encode.enc.*` (width c_dim, on 2x - 1 where do_center) gives ctx; aux_encode is a Gaussian head on ctx
    (z0 of width z0_dim = `noise_dim`, no log-variance clip), encode `fc.0` + ELU on cat[ctx, z0] and a head on z, aux_decode `fc.0` + ELU on cat[ctx, z]
    and a head on z0; MNISTResConvVAE's decoder.  ELU only (vae/auxresconv.py:278), 28x28x1 only.  forward() takes x as [B, 784] or [B, 1, 28, 28] and
    returns the decoder sample / mean as [B, 784]."""
    _kind = "vae_auxresconv"
    # As for MNISTResConvVAE the library picks the kernel of every conv-as-linear by the row count, so the evaluator runs fixed groups: the statistics and
    # the ELBO pass on 64 images per call, the three stages and the importance samples' decoder on 16.  The decode-only workspace of this kind (one
    # columns scratch sized from the 8 x 8 blocks, the 14 x 14 stage and the last stage fused) takes ~5.3e4 floats per decoded row against ~1.18e5
    # for MNISTResConvVAE's: at k = 256 the 4096 rows of a call need 0.22 G floats, inside the default budget of 2^28 (32 images would need 0.43 G).
    # Chunks are cut at multiples of 64 images.
    _eval_groups = (64, 16)

    def __init__(self, energy_func=normal_energy_func, input_height=28, input_channels=1, z0_dim=100, z_dim=32, c_dim=450, nonlinearity="elu",
                 do_center=False):
        if input_height != 28 or input_channels != 1:
            raise NotImplementedError("MNISTResConvAuxVAE: the reference asserts 28x28x1 (models/vae/auxresconv.py:276-277)")
        if nonlinearity != "elu":
            raise NotImplementedError(f"MNISTResConvAuxVAE: nonlinearity {nonlinearity!r}: the reference asserts 'elu' (models/vae/auxresconv.py:278)")
        super().__init__()
        self.input_height, self.input_channels, self.c_dim, self.z0_dim = input_height, input_channels, int(c_dim), int(z0_dim)
        self.do_center = bool(do_center)
        if not 1 <= int(z0_dim) <= 128:
            raise ValueError(f"MNISTResConvAuxVAE: noise_dim must be 1 .. 128 (got {z0_dim})")
        self.noise_dim, self.enc_type, self.clip_logvar = int(z0_dim), "simple", None
        self._build(energy_func, input_height * input_height * input_channels, c_dim, z_dim, nonlinearity, 1, 0 if do_center else L.MODEL_NO_CENTER,
                    noise_dim=self.noise_dim, boxes={})

    def _param_spec(self):
        return layout.aux_resconv_vae_spec(self.noise_dim, self.z_dim, self.c_dim)

    def reset_parameters(self):
        self._default_init()                                # the two fc.0 and the six heads: nn.Linear's default
        with torch.no_grad():
            _weight_norm_init(dict(self._spec), dict(self.named_parameters()))
