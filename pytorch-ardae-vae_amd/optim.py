"""Optimisers of the reference loop as fused multi-tensor HIP updates.

    Adam    <- utils/optim.py:9-108 (vendored old-style Adam: `denom = (sqrt(v) + eps) / sqrt(1 - beta2^t)`, :102-106)
    RMSprop <- torch.optim.RMSprop as constructed at ivae_ardae.py:625-626 (momentum form, alpha=.99, eps=1e-8)

Same constructor signatures, `param_groups`, `state_dict()` layout (`exp_avg`, `exp_avg_sq`, `step`, `max_exp_avg_sq`;
`square_avg`, `momentum_buffer`, `step`).  Parameters that are adjacent views of one flat buffer (the modules in
modules.py) and whose gradients are adjacent too are updated by ONE kernel launch per run; a parameter whose `.grad`
is None is skipped and keeps no state, exactly like the reference (`neglogprob.fc.bias`).
"""
import torch
from torch.optim.optimizer import Optimizer

from . import _lib as L


def _runs(params):
    """Group (param, grad, state tensors...) tuples into maximal runs that are contiguous in memory."""
    runs, cur = [], None
    for tensors in params:
        if cur is not None and all(c[-1].data_ptr() + c[-1].numel() * 4 == t.data_ptr() for c, t in zip(cur, tensors)):
            for c, t in zip(cur, tensors):
                c.append(t)
        else:
            if cur is not None:
                runs.append(cur)
            cur = [[t] for t in tensors]
    if cur is not None:
        runs.append(cur)
    return runs


def _bump(p):
    torch.autograd.graph.increment_version(p)


class _FlatStateOptimizer(Optimizer):
    _state_names = ()

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        # these optimisers bump the parameters' version counters after every step, so the owning modules may keep their packed
        # weight image until a version moves instead of rebuilding it at every forward (modules.py::FlatParamModule._pack_is_current)
        for group in self.param_groups:
            for p in group["params"]:
                owner = getattr(p, "_ardae_owner", None)
                owner = owner() if owner is not None else None
                if owner is not None:
                    owner._tracked = True

    def _state_for(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            for n in self._state_names(p):
                st[n] = None
        return st

    def _alloc_states(self, group_params, names):
        """Allocate state tensors of consecutive parameters as views of one buffer so the update stays one launch."""
        need = [p for p in group_params if any(self.state[p].get(n) is None for n in names)]
        if not need:
            return
        total = sum(p.numel() for p in need)
        for n in names:
            buf = torch.zeros(total, device=need[0].device, dtype=torch.float32)
            off = 0
            for p in need:
                self.state[p][n] = buf[off:off + p.numel()].view_as(p)
                off += p.numel()


class Adam(_FlatStateOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if weight_decay != 0:
            raise NotImplementedError("weight_decay != 0 is never used by ivae_ardae.py and is not implemented on the HIP path")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))

    def _state_names(self, p):
        return ("exp_avg", "exp_avg_sq")

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            active = [p for p in group["params"] if p.grad is not None]
            if not active:
                continue
            names = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if group["amsgrad"] else [])
            for p in active:
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                self._state_for(p)
                for n in names:
                    self.state[p].setdefault(n, None)
            self._alloc_states(active, names)
            # parameters that share a step count and sit next to each other go out in one launch
            tuples = []
            for p in active:
                st = self.state[p]
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                tuples.append((p.data, g, st["exp_avg"], st["exp_avg_sq"]) + ((st["max_exp_avg_sq"],) if group["amsgrad"] else ()) )
            steps = [self.state[p]["step"] for p in active]
            start = 0
            while start < len(active):
                end = start
                while end < len(active) and steps[end] == steps[start]:
                    end += 1
                for run in _runs(tuples[start:end]):
                    n = sum(t.numel() for t in run[0])
                    vmax = run[4][0] if group["amsgrad"] else None
                    L.call("ardae_adam_ref_step", run[0][0], run[1][0], run[2][0], run[3][0], vmax, n, float(group["lr"]),
                           float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), int(steps[start]))
                start = end
            for p in active:
                _bump(p)
        return loss


class RMSprop(_FlatStateOptimizer):
    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= momentum:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if not 0.0 <= alpha:
            raise ValueError("Invalid alpha value: {}".format(alpha))
        if weight_decay != 0 or centered:
            raise NotImplementedError("weight_decay / centered RMSprop are never used by ivae_ardae.py and are not implemented on the HIP path")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered))

    def _state_names(self, p):
        return ("square_avg", "momentum_buffer")

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            active = [p for p in group["params"] if p.grad is not None]
            if not active:
                continue
            names = ["square_avg"] + (["momentum_buffer"] if group["momentum"] > 0 else [])
            for p in active:
                self._state_for(p)
                for n in names:
                    self.state[p].setdefault(n, None)
            self._alloc_states(active, names)
            tuples = []
            for p in active:
                st = self.state[p]
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                tuples.append((p.data, g, st["square_avg"]) + ((st["momentum_buffer"],) if group["momentum"] > 0 else ()))
            for run in _runs(tuples):
                n = sum(t.numel() for t in run[0])
                buf = run[3][0] if group["momentum"] > 0 else None
                L.call("ardae_rmsprop_step", run[0][0], run[1][0], run[2][0], buf, n, float(group["lr"]), float(group["alpha"]),
                       float(group["eps"]), float(group["momentum"]))
            for p in active:
                _bump(p)
        return loss


# ------------------------------------------------------------------------------------------------------------------------------
# Weight averaging of the model parameters: --m-weight-avg polyak | swa (ivae_ardae.py:158-164,559-565,646-647,671-672, where the
# model optimiser is wrapped in torchcontrib.optim.Polyak / SWA).  torchcontrib is a VCS dependency that is not importable here, so its
# rules are restated as this project's definition, after upstream torchcontrib's SWA in automatic mode with freq 1 (the only freq the
# script passes):
#   t = steps of the wrapped optimiser, the current one included; averaging happens at every step with t > start;
#   k = t - (start + 1) = earlier averaging steps
#   SWA:    avg += (p - avg) * (1 / (k + 1))                    (k = 0: avg = p exactly)
#   Polyak: k = 0: avg = p exactly;  k > 0: avg += (p - avg) * (1 - decay)
#   w is rounded to fp32 and the update keeps the order avg + (p - avg) * w (kernel: ardae_weight_avg).  Before the first averaging
#   step there is no buffer: use_buf() then leaves the raw weights in place, as torchcontrib's swap does when it finds none.
# Checkpoint layout: upstream SWA.state_dict() with parameter INDICES as keys (upstream uses id(tensor), which does not survive a file):
#   {"opt_state": <inner optimizer's state>, "swa_state" | "polyak_state": {idx: {"swa_buffer" | "polyak_buffer": tensor}},
#    "param_groups": <inner optimizer's groups, each with "n_avg" (averaging steps done) and "step_counter" (t)>}
# The Polyak key names are an assumption (the fork that adds Polyak is not available to compare against).
WEIGHT_AVG_KINDS = {"swa": L.WEIGHT_AVG_SWA, "polyak": L.WEIGHT_AVG_POLYAK}


def weight_avg_keys(kind):
    """("<kind>_state", "<kind>_buffer"): the two key names of the wrapper layout."""
    return f"{kind}_state", f"{kind}_buffer"


def wrap_state_dict(inner, kind, buffers):
    """A torch.optim state_dict ({"state", "param_groups"}, groups already carrying n_avg / step_counter) and the averaged buffers
    {param index: tensor} -> the wrapper layout above."""
    if kind not in WEIGHT_AVG_KINDS:
        raise NotImplementedError(f"unknown weight averaging: {kind}")
    skey, bkey = weight_avg_keys(kind)
    return {"opt_state": inner["state"], skey: {int(i): {bkey: b} for i, b in buffers.items()}, "param_groups": inner["param_groups"]}


def unwrap_state_dict(sd):
    """Inverse of wrap_state_dict: (inner torch.optim state_dict, kind, {param index: buffer}).  A plain optimiser state_dict passes
    through as (sd, None, {})."""
    if "opt_state" not in sd:
        return sd, None, {}
    kinds = [k for k in WEIGHT_AVG_KINDS if weight_avg_keys(k)[0] in sd]
    if len(kinds) != 1:
        raise ValueError(f"wrapped optimiser state with {'no' if not kinds else 'more than one'} averaging state ({sorted(sd)})")
    kind = kinds[0]
    skey, bkey = weight_avg_keys(kind)
    bufs = {int(i): st[bkey] for i, st in sd[skey].items() if st.get(bkey) is not None}
    return {"state": sd["opt_state"], "param_groups": sd["param_groups"]}, kind, bufs


class _WeightAverage:
    """torchcontrib.optim.SWA / Polyak (automatic mode, freq 1) around an optimiser over this package's modules (net.Adam, net.RMSprop,
    or any torch optimiser).  The buffers of a param group are views of one allocation laid out like the parameters, so a run of
    parameters that are adjacent in memory (a module's flat buffer) is averaged by ONE `ardae_weight_avg` launch."""

    def __init__(self, optimizer, kind, start, freq, decay=None):
        if kind not in WEIGHT_AVG_KINDS:
            raise NotImplementedError(f"unknown weight averaging: {kind}")
        if freq != 1:
            raise NotImplementedError(f"{kind} freq {freq}: only freq 1 is implemented (ivae_ardae.py:561,563 always passes 1)")
        if start is None or int(start) < 0:
            raise ValueError(f"{kind} start must be an int >= 0 (manual mode is not implemented), got {start!r}")
        if decay is not None and not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"invalid Polyak decay: {decay}")
        self.optimizer, self.kind, self.start = optimizer, kind, int(start)
        self.decay = 0.0 if decay is None else float(decay)
        self.state = {}             # param -> {"<kind>_buffer": tensor}
        self._swapped = None        # inside use_buf(): the parameters whose values were swapped with their buffers
        for group in self.param_groups:
            group.setdefault("n_avg", 0)
            group.setdefault("step_counter", 0)

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    @property
    def defaults(self):
        return self.optimizer.defaults

    def zero_grad(self, set_to_none=True):
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def _buffer(self, p):
        return self.state.get(p, {}).get(weight_avg_keys(self.kind)[1])

    def _alloc(self, params):
        """Buffers for `params` as views of one allocation whose 16-byte phase matches the first parameter's (float4 path)."""
        bkey = weight_avg_keys(self.kind)[1]
        need = [p for p in params if self._buffer(p) is None]
        if not need:
            return
        total = sum(p.numel() for p in need)
        raw = torch.zeros(total + 3, device=need[0].device, dtype=torch.float32)
        off = ((need[0].data_ptr() - raw.data_ptr()) // 4) % 4
        for p in need:
            self.state.setdefault(p, {})[bkey] = raw[off:off + p.numel()].view_as(p)
            off += p.numel()

    @torch.no_grad()
    def step(self, closure=None):
        if self._swapped is not None:
            raise RuntimeError(f"{type(self).__name__}.step() while the averaged weights are in: call use_sgd() first")
        loss = self.optimizer.step(closure)
        for group in self.param_groups:
            group["step_counter"] += 1
            t = group["step_counter"]
            if t <= self.start:
                continue
            params = list(group["params"])
            self._alloc(params)
            origin = t - group["n_avg"]          # k = t - origin = averaging steps already in the buffers
            for run in _runs([(p.data, self._buffer(p)) for p in params]):
                n = sum(x.numel() for x in run[0])
                L.call("ardae_weight_avg", run[1][0], run[0][0], n, WEIGHT_AVG_KINDS[self.kind], self.decay, origin, None, t)
            group["n_avg"] += 1
        return loss

    @torch.no_grad()
    def _swap(self, params):
        for p in params:
            buf = self._buffer(p)
            tmp = p.data.clone()
            p.data.copy_(buf)
            buf.copy_(tmp)
            _bump(p)                 # the owning module re-packs its weight image at its next use

    def use_buf(self):
        """ivae_ardae.py:646-647: the averaged weights into the parameters (in place); parameters without a buffer (no averaging step
        yet) keep their raw values."""
        if self._swapped is not None:
            return
        self._swapped = [p for g in self.param_groups for p in g["params"] if self._buffer(p) is not None]
        self._swap(self._swapped)

    def use_sgd(self):
        """ivae_ardae.py:671-672: the raw weights back, bit for bit."""
        if self._swapped is None:
            return
        self._swap(self._swapped)
        self._swapped = None

    def state_dict(self):
        if self._swapped is not None:
            raise RuntimeError(f"{type(self).__name__}.state_dict() while the averaged weights are in: call use_sgd() first")
        bufs, i = {}, 0
        for g in self.param_groups:
            for p in g["params"]:
                if self._buffer(p) is not None:
                    bufs[i] = self._buffer(p)
                i += 1
        return wrap_state_dict(self.optimizer.state_dict(), self.kind, bufs)

    def load_state_dict(self, state_dict):
        """The wrapper layout (this wrapper's or the fused engine's model_checkpoint()['optimizer']) or a plain optimiser state_dict; a
        plain one past `start` starts a fresh average at the next step."""
        if self._swapped is not None:
            raise RuntimeError(f"{type(self).__name__}.load_state_dict() while the averaged weights are in: call use_sgd() first")
        inner, kind, bufs = unwrap_state_dict(state_dict)
        if kind is not None and kind != self.kind:
            raise ValueError(f"the state holds a {kind!r} average, this wrapper is {self.kind!r}")
        self.optimizer.load_state_dict(inner)
        self.state = {}
        i = 0
        for group in self.param_groups:
            steps = [int(st["step"]) for p in group["params"] for st in (self.optimizer.state.get(p, {}),) if "step" in st]
            group.setdefault("step_counter", max(steps) if steps else 0)
            if kind is None:
                group["n_avg"] = 0
            group.setdefault("n_avg", 0)
            params = list(group["params"])
            mine = [p for k, p in enumerate(params, i) if k in bufs]
            if group["n_avg"] and len(mine) != len(params):
                raise ValueError(f"{self.kind} state: {group['n_avg']} averaging steps recorded but buffers for {len(mine)} of {len(params)} parameters")
            self._alloc(mine)
            with torch.no_grad():
                for k, p in enumerate(params, i):
                    if k in bufs:
                        self._buffer(p).copy_(bufs[k])
            i += len(params)


class Polyak(_WeightAverage):
    """torchcontrib.optim.Polyak(optimizer, polyak_start, polyak_freq=1, polyak_decay) as built at ivae_ardae.py:561 (decay default:
    the script's --m-weight-avg-decay default)."""

    def __init__(self, optimizer, polyak_start, polyak_freq=1, polyak_decay=0.998):
        super().__init__(optimizer, "polyak", polyak_start, polyak_freq, polyak_decay)


class SWA(_WeightAverage):
    """torchcontrib.optim.SWA(optimizer, swa_start, swa_freq=1) as built at ivae_ardae.py:563 (no swa_lr: the script passes none)."""

    def __init__(self, optimizer, swa_start, swa_freq=1, swa_lr=None):
        if swa_lr is not None:
            raise NotImplementedError("swa_lr (SWA's learning-rate schedule) is never used by ivae_ardae.py and is not implemented")
        super().__init__(optimizer, "swa", swa_start, swa_freq)
