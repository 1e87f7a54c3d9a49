"""Host logic the engines (engine.py, score_engine.py, fit.py, vae.py) share: the Philox stride of a step, argument validation, graph capture,
the flat optimiser and its checkpoint."""
import torch

from . import _lib as L

RNG_STRIDE = 16   # Philox offsets reserved per step (draws use base + 0, 1, 2, ...)


# ---- validation: nothing unchecked reaches a kernel pointer ---------------------------------------------------------------------------
def check_tensor(t, what, dev, shape=None, numel=None):
    """`t` must be a contiguous float32 tensor on `dev` with exactly `shape` (None entries: any size), or - shape None - `numel` values."""
    if not torch.is_tensor(t):
        why = f"got a {type(t).__name__}"
    elif t.dtype != torch.float32:
        why = f"got {t.dtype}"
    elif t.numel() != numel if shape is None else t.dim() != len(shape) or any(w not in (None, g) for w, g in zip(shape, t.shape)):
        why = f"got shape {list(t.shape)}"
    elif not t.is_contiguous():
        why = f"got strides {tuple(t.stride())}; call .contiguous()"
    elif not t.is_cuda or t.device != dev:
        why = f"expected a tensor on {dev}, got one on {t.device}"
    else:
        return
    size = f"{numel} values" if shape is None else f"shape {list(shape)}"
    raise ValueError(f"{what} must be a contiguous float32 tensor of {size} on {dev}: {why}")


def check_batch(x, what, dev, B, width, rows="samples"):
    """The kernels read exactly B * width contiguous floats from a batch pointer: anything else (a ragged last batch of a loader without
    drop_last, a strided view, a host tensor) is refused here, not read out of bounds.  Image-shaped batches [B, C, H, W] pass."""
    if not torch.is_tensor(x):
        raise TypeError(f"{what}: expected a tensor, got {type(x).__name__}")
    if x.dim() < 2 or x.size(0) != B or x.numel() != B * width:
        raise ValueError(f"{what}: expected {B} {rows} of {width} values (the engine was built with batch_size={B}; use drop_last or pad the "
                         f"last batch), got shape {tuple(x.shape)}")
    check_tensor(x, what, dev, numel=B * width)


def bump_versions(module):
    """The parameters were written by a kernel: the module path (modules.py, `_pack_is_current`) re-packs at its next use."""
    for p in module.parameters():
        torch.autograd.graph.increment_version(p)


def rebuild_step_state(block, n, stride, advance):
    """A step block that was not saved, after `n` steps: Philox offsets the run has not used and t = n, advanced to describe the coming step."""
    block.zero_()
    block[0], block[1] = stride * n, n
    advance()


def capture_linear(fns, stream):
    """The launches of `fns` as ONE linear HIP graph, captured on `stream` (the default stream cannot capture).  A capture runs nothing."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for fn in fns:
            fn()
    return g


class CaptureLadder:
    """An engine whose step is one linear graph: the first two calls run eagerly (every kernel is loaded outside of a capture), the third
    is captured and replayed once, later ones replay.  `eager=True` (injected noise) and graph=False run the launches as they are; every
    call counts.  `reset()`: the captured launches no longer describe the step (a checkpoint was loaded)."""

    def __init__(self, dev, graph):
        if graph not in (True, False):
            raise ValueError(f"graph must be True or False, got {graph!r}")
        self.on = bool(graph) and L.debug_knob("ARDAE_GRAPH", "1") != "0"
        self.stream = torch.cuda.Stream(device=dev)
        self.reset()

    def reset(self):
        self.graph, self.calls = None, 0

    def run(self, body, eager=False):
        if eager or not self.on or (self.graph is None and self.calls < 2):
            body()
        else:
            g = self.graph or capture_linear([body], self.stream)
            g.replay()
            self.graph = g
        self.calls += 1


class _FlatOpt:
    """One network's optimiser on its flat parameter / gradient buffers: torch.optim.SGD(lr), the reference's vendored Adam (amsgrad
    optional; utils/optim.py:49-108) or torch.optim.RMSprop(momentum) - the four choices of --m-optimizer / --d-optimizer.  `n`: floats
    that receive gradients (a grad-kind score network's trailing neglogprob.fc.bias does not and keeps no state).  Adam's t and bias
    corrections live in a 32-byte device block (`ardae_step_state_advance`) so that a captured step can be replayed.  `train`:
    (beta_init, beta_fin, beta_annealing, std_scale, seed_rows) of a beta schedule - the block is then advanced by
    `ardae_train_state_advance`, which also writes the coming step's beta and entropy-seed factor into its last 8 bytes.  `dae`:
    (sigma_max, sigma_min, sigma_annealing) of notebooks/dae_toy.ipynb's noise schedule - the block is advanced by
    `ardae_dae_state_advance`, which writes the coming step's sigma there.  'adam_torch' is torch.optim.Adam (epsilon after the bias
    correction; `ardae_adam_torch_step_dev`): it reads the device block, so it runs inside an engine's step only."""
    KINDS = ("sgd", "adam", "amsgrad", "rmsprop", "adam_torch")

    def __init__(self, kind, flat, n, lr, beta1, momentum, state=None, train=None, dae=None):
        if kind not in self.KINDS:
            raise NotImplementedError(f"unknown optimizer: {kind}")                     # ivae_ardae.py:555-556,621-622
        self.kind, self.flat, self.n, self.lr, self.beta1, self.momentum = kind, flat, int(n), float(lr), float(beta1), float(momentum)
        z = lambda: torch.zeros_like(flat)
        self.a = None if kind == "sgd" else z()                                         # exp_avg | square_avg
        self.b = None if kind == "sgd" else z()                                         # exp_avg_sq | momentum_buffer
        self.c = z() if kind == "amsgrad" else None                                     # max_exp_avg_sq
        self.steps, self.train, self.dae = 0, train, dae
        self.state = state if state is not None else torch.zeros(4, dtype=torch.int64, device=flat.device)

    @property
    def adam(self):
        return self.kind in ("adam", "amsgrad", "adam_torch")

    def advance(self, rng_inc=0):
        if self.train is not None:
            L.call("ardae_train_state_advance", self.state, rng_inc, self.lr, self.beta1, 0.999, *self.train)
        elif self.dae is not None:
            L.call("ardae_dae_state_advance", self.state, rng_inc, self.lr, self.beta1, 0.999, *self.dae)
        else:
            L.call("ardae_step_state_advance", self.state, rng_inc, self.lr, self.beta1, 0.999)

    def apply(self, grads, in_step):
        p, g = self.flat, grads
        if self.kind == "sgd":
            L.call("ardae_sgd_step", p, g, self.n, self.lr)
        elif self.kind == "rmsprop":
            L.call("ardae_rmsprop_step", p, g, self.a, self.b, self.n, self.lr, 0.99, 1e-8, self.momentum)
        elif self.kind == "adam_torch":
            if not in_step:
                raise NotImplementedError("adam_torch takes t and its bias corrections from the device block: it runs inside an engine's step")
            L.call("ardae_adam_torch_step_dev", p, g, self.a, self.b, self.n, self.beta1, 0.999, 1e-8, self.state)
        elif in_step:      # t and the bias corrections come from the device block (advanced inside the step)
            L.call("ardae_adam_ref_step_dev", p, g, self.a, self.b, self.c, self.n, self.beta1, 0.999, 1e-8, self.state)
        else:
            L.call("ardae_adam_ref_step", p, g, self.a, self.b, self.c, self.n, self.lr, self.beta1, 0.999, 1e-8, self.steps + 1)

    # torch.optim.Optimizer.state_dict() layout (per-parameter views of the flat buffers), so that files written by the reference loop, by
    # the drop-in modules + net.Adam / net.RMSprop, and by the engines are interchangeable
    def state_names(self):
        return {"sgd": (), "adam": ("exp_avg", "exp_avg_sq"), "adam_torch": ("exp_avg", "exp_avg_sq"), "amsgrad": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"),
                "rmsprop": ("square_avg", "momentum_buffer")}[self.kind]

    def buffers(self):
        return [t for t in (self.a, self.b, self.c) if t is not None]

    def param_group(self, nparams):
        if self.kind == "sgd":
            g = {"lr": self.lr, "momentum": 0, "dampening": 0, "weight_decay": 0, "nesterov": False}
        elif self.adam:
            g = {"lr": self.lr, "betas": (self.beta1, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": self.kind == "amsgrad"}
        else:
            g = {"lr": self.lr, "momentum": self.momentum, "alpha": 0.99, "eps": 1e-8, "centered": False, "weight_decay": 0}
        g["params"] = list(range(nparams))
        return g

    @staticmethod
    def _kind_of_group(group):
        """Which optimiser wrote this torch.optim param_group (utils.Adam / torch.optim.RMSprop / torch.optim.SGD layouts)."""
        if "betas" in group:
            return "amsgrad" if group.get("amsgrad") else "adam"
        return "rmsprop" if "alpha" in group else "sgd"

    def state_dict(self, module):
        """{'state': {param index: {'step', <this optimiser's buffers>}}, 'param_groups'} for `module`, whose parameters `flat` holds;
        parameters without gradients and optimisers without state (SGD, or no step yet) contribute no entry."""
        names, state = self.state_names(), {}
        if self.steps and names:
            views = [module.param_views(t, grads_only=True) for t in self.buffers()]
            for i, first in enumerate(views[0]):
                if first is not None:
                    state[i] = dict({"step": self.steps}, **{nm: v[i].clone() for nm, v in zip(names, views)})
        return {"state": state, "param_groups": [self.param_group(len(list(module.named_parameters())))]}

    def load_state_dict(self, module, sd, what):
        """Inverse of state_dict(), also for what torch.optim and the reference's optimisers write.  -> the step count found (0: empty state)."""
        state, groups = sd["state"], sd.get("param_groups")
        # (torch.optim.Adam and the vendored Adam write the same param_group: either file loads into 'adam' and 'adam_torch')
        if groups and self._kind_of_group(groups[0]) != ("adam" if self.kind == "adam_torch" else self.kind):
            raise ValueError(f"{what}: written by optimiser {self._kind_of_group(groups[0])!r}, but this engine was built with {self.kind!r} for that network")
        for t in self.buffers():
            t.zero_()
        steps = {int(st["step"]) for st in state.values()}
        if len(steps) > 1:
            raise ValueError(f"the fused engine keeps one step count per network ({what}: {sorted(steps)})")
        names = self.state_names()
        if state and not all(nm in next(iter(state.values())) for nm in names[:1]):
            raise ValueError(f"{what}: the checkpoint's optimiser state does not belong to {self.kind!r}")
        with torch.no_grad():
            for nm, buf in zip(names, self.buffers()):
                for i, t in enumerate(module.param_views(buf, grads_only=True)):
                    if t is not None and i in state and state[i].get(nm) is not None:
                        t.copy_(state[i][nm])
        return steps.pop() if steps else 0
