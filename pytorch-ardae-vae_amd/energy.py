"""utils/energy.py on the device: regularization_func, energy_func1..4 and normal_energy_func as callables on GPU tensors.

Each call is one launch of the energy kernel (csrc/energy.hip), which returns the energies and the analytic gradient dE/dx together;
autograd receives that gradient (`_EnergyFn`), so `torch.mean(energy_func4(x)).backward()` - the generator's loss of
notebooks/ardae_fit.ipynb - runs no PyTorch arithmetic on the rows.  Shapes follow the reference: [R, 1] for regularization_func and
energy_func1..4, [R] for normal_energy_func.  The kernel takes and returns fp32: an input of another floating dtype is converted, the energies come back as
float32 whatever the input was (the reference returns the input's dtype), the gradient in the input's dtype.  The gradient is a stored
tensor, so the functions are ONCE differentiable (a double backward raises instead of returning zeros).  There is no CPU path.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

KINDS = {"reg": L.CONSTANTS["ARDAE_ENERGY_REG"], "energy_func1": L.CONSTANTS["ARDAE_ENERGY_1"], "energy_func2": L.CONSTANTS["ARDAE_ENERGY_2"],
         "energy_func3": L.CONSTANTS["ARDAE_ENERGY_3"], "energy_func4": L.CONSTANTS["ARDAE_ENERGY_4"],
         "normal_energy_func": L.CONSTANTS["ARDAE_ENERGY_NORMAL"]}


def _rows(x, kind):
    if not torch.is_tensor(x):
        raise TypeError(f"expected a tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError(f"net.energy: got a {x.device} tensor; inputs must be on the GPU (there is no CPU path)")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"net.energy: expected a non-empty batch, got shape {tuple(x.shape)}")
    if KINDS["energy_func1"] <= kind <= KINDS["energy_func4"]:
        assert x.dim() == 2                # utils/energy.py:20-21
        assert x.size(1) == 2
    return x.detach().to(torch.float32).contiguous()


def evaluate(kind, x, mu=0., logvar=0., want_grad=True):
    """-> (energies [R], dE/dx [R, d] or None) of x [R, d] (contiguous fp32 on the GPU) through the C ABI."""
    R, d = x.size(0), x.numel() // x.size(0)
    e = torch.empty(R, device=x.device, dtype=torch.float32)
    g = torch.empty(R, d, device=x.device, dtype=torch.float32) if want_grad else None
    L.call("ardae_energy", kind, x, R, d, float(mu), float(logvar), e, g)
    return e, g


class _EnergyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, mu, logvar):
        rows = _rows(x, kind)
        if kind == KINDS["reg"]:           # elementwise in the reference: every leading dimension is a batch dimension
            rows = rows.view(-1, x.size(-1))
        e, g = evaluate(kind, rows, mu, logvar, want_grad=x.requires_grad)
        ctx.g, ctx.shape, ctx.dtype = g, x.shape, x.dtype
        return e

    @staticmethod
    @once_differentiable
    def backward(ctx, ge):
        return (ge.reshape(-1, 1) * ctx.g).reshape(ctx.shape).to(ctx.dtype), None, None, None


def regularization_func(x):
    """utils/energy.py:7-8: (relu(|x| - 6)^2).sum(-1, keepdim=True)."""
    return _EnergyFn.apply(x, KINDS["reg"], 0., 0.).view(*x.shape[:-1], 1)


def energy_func1(x):
    return _EnergyFn.apply(x, KINDS["energy_func1"], 0., 0.).view(-1, 1)


def energy_func2(x):
    return _EnergyFn.apply(x, KINDS["energy_func2"], 0., 0.).view(-1, 1)


def energy_func3(x):
    return _EnergyFn.apply(x, KINDS["energy_func3"], 0., 0.).view(-1, 1)


def energy_func4(x):
    return _EnergyFn.apply(x, KINDS["energy_func4"], 0., 0.).view(-1, 1)


def normal_energy_func(x, mu=0., logvar=0.):
    """utils/energy.py:74-77: sum over all but the batch dimension of 0.5 (logvar + (x - mu)^2 / exp(logvar) + log 2 pi)."""
    return _EnergyFn.apply(x, KINDS["normal_energy_func"], mu, logvar)


def kind_of(energy):
    """ARDAE_ENERGY_* of a name ('energy_func4'), of one of this module's callables, or of the number itself."""
    if callable(energy):
        energy = getattr(energy, "__name__", None)
    if isinstance(energy, str) and energy in KINDS and energy != "reg":
        return KINDS[energy]
    if isinstance(energy, int) and not isinstance(energy, bool) and energy in KINDS.values() and energy != KINDS["reg"]:
        return energy
    raise NotImplementedError(f"energy {energy!r}: utils/energy.py has energy_func1 .. energy_func4 and normal_energy_func")
