"""What the CPU tests of the six Gaussian VAE families (tests/test_vae_{,conv_,resconv_,aux_,auxconv_,auxresconv_}baseline.py) share, written once:
fixtures, the float64 tolerance, the reference's Adam, tensor summaries, the KL / log-density rows, the importance-weight logsumexp, the float64
trajectory loop - and the pieces of one family's float64 restatement that another family needs (the conv and residual-conv trunks and decoders,
the numpy restatement of the MLP auxiliary family).  Not a test module: nothing here is collected, so every assertion carries its message.

Functions that take `p` take {name: tensor}; the torch ones take float64 tensors (autograd gives the gradients), the `aux_` ones float64 numpy
arrays (the backward is written out).  `lin`, `adam_step`, `summary`, the KL rows and `iw_logsumexp` take either."""
import glob
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O
from score_restate import ACTS, rel  # noqa: F401  (re-exported: the family files take them from here)

BETAS = {"b1": 1.0, "b03": 0.3}
TOL64 = 1e-9          # float64 restatement against the reference's float64 outputs: losses, full tensors and summaries
LOG_2PI = math.log(2 * math.pi)
D28 = 784             # the image families' input_dim


def load(golden_dir, name):
    """A fixture and its parts (<name>.npz, <name>.p1.npz, ...: tools/gen_vae_golden.py::save_split) as one dict."""
    paths = [os.path.join(golden_dir, name + ".npz")] + sorted(glob.glob(os.path.join(golden_dir, name + ".p*.npz")))
    fx = {}
    for p in paths:
        fx.update(np.load(p))
    return fx


def t64(a):
    """-> a float64 torch tensor on the host"""
    return a.detach().double().cpu() if torch.is_tensor(a) else torch.tensor(np.asarray(a)).double()


def _exp(v):
    return v.exp() if torch.is_tensor(v) else np.exp(v)


def fails(rc, fragment):
    """a C ABI call refused its arguments, and ardae_last_error says why"""
    err = L.lib().ardae_last_error()
    assert rc < 0, (fragment, rc)
    assert fragment.encode() in err, (fragment, err)


def traj_config(fx, **kw):
    return net.VaeConfig(lr=float(fx["cfg/lr"]), beta1=float(fx["cfg/beta1"]), beta_init=float(fx["cfg/beta_init"]), beta_fin=float(fx["cfg/beta_fin"]),
                         beta_annealing=int(fx["cfg/beta_annealing"]), **kw)


# ---- pieces every restatement is made of ---------------------------------------------------------------------------------------------
def lin(p, name, hdn):
    return hdn @ p[name + ".weight"].T + p[name + ".bias"]


def kld_rows(mu, lv):
    return -0.5 * (1 + lv - mu ** 2 - _exp(lv)).sum(1)                                              # utils/vae.py:78-92


def pair_kld_rows(mu1, lv1, mu2, lv2):
    return -0.5 * (1 - lv2 + lv1 - (_exp(lv1) + (mu1 - mu2) ** 2) / _exp(lv2)).sum(1)               # utils/vae.py:94-114


def log_normal_rows(v, mu, lv):
    return (-0.5 * ((v - mu) ** 2 / _exp(lv) + lv + LOG_2PI)).sum(-1)                               # utils/stat.py:65-85


def relaxed_sample(logit, u):
    """BernoulliDistribution.sample_logistic_sigmoid at temperature 1 on the uniform draw u (models/reparam.py:111-120)"""
    return torch.sigmoid(logit + torch.log(u + 1e-20) - torch.log(1 - u + 1e-20))


def iw_logsumexp(lw):
    """What every VAE.logprob ends with: log mean exp over the k importance weights lw [B, k], the maximum taken out, 1e-10 inside the log -> [B]"""
    t = torch.as_tensor(lw)
    m = t.max(1, keepdim=True)[0]
    out = (torch.log(torch.mean((t - m).exp(), 1, keepdim=True) + 1e-10) + m).view(-1)
    return out if torch.is_tensor(lw) else out.numpy()


def gaussian_logprob_rows(mu, lv, x, eps, recon):
    """VAE.logprob before its mean for the families with one Gaussian stage (vae/mnist.py:179-217, vae/conv.py:218-257, vae/resconv.py:198-240)
    on injected draws eps [B, k, zd]; recon(x rows, z rows) -> -log p(x | z) per row"""
    B, k, zd = eps.shape
    mu, lv = mu[:, None, :], lv[:, None, :]
    z = mu + torch.exp(0.5 * lv) * eps
    logq = log_normal_rows(z, mu, lv)
    logprior = (-0.5 * (z ** 2 + LOG_2PI)).sum(2)
    rec = recon(x[:, None, :].expand(B, k, x.size(1)).reshape(B * k, -1), z.reshape(B * k, zd))
    return iw_logsumexp(-rec.view(B, k) + logprior - logq)


def loss_and_grads(forward, p, *args, scale):
    """-> forward(p, *args)'s dict (detached) and {name: d (scale * loss) / d p}, with clones of p's tensors as the leaves"""
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = forward(p, *args)
    grads = dict(zip(p, torch.autograd.grad(scale * out["loss"], list(p.values()))))
    return {k: v.detach() for k, v in out.items()}, grads


def adam_step(p, g, st, lr, beta1, t):
    """The reference's vendored Adam (utils/optim.py:84-106: epsilon before the bias correction), in place"""
    bc1, bc2 = 1 - beta1 ** t, 1 - 0.999 ** t
    for k in p:
        m, v = st.setdefault(k, (0 * p[k], 0 * p[k]))
        m *= beta1
        m += (1 - beta1) * g[k]
        v *= 0.999
        v += (1 - 0.999) * g[k] * g[k]
        p[k] -= lr / bc1 * m / ((v ** 0.5 + 1e-8) / math.sqrt(bc2))


def trajectory(fx, p, step_fn):
    """A trajectory fixture's loop restated in float64: step_fn(p, x, eps, beta) -> (forward's dict, gradients) on the fixture's arrays; yields
    (step, forward's dict, the parameters after the vendored Adam's step)"""
    cfg, st = traj_config(fx), {}
    for s in range(int(fx["cfg/steps"])):
        beta = cfg.beta_at(s)
        assert beta == float(fx[f"{s}/beta"]), ("beta of step", s, beta)
        out, grads = step_fn(p, fx[f"{s}/x"], fx[f"{s}/eps"], beta)
        adam_step(p, grads, st, cfg.lr, cfg.beta1, s + 1)
        yield s, out, p


def summary(t):
    """What a fixture keeps of a large tensor: [L2 norm, sum, the first 8 elements]"""
    t = torch.as_tensor(t).detach().reshape(-1)
    return torch.cat([torch.stack([t.norm(), t.sum()]), t[:8]])


def summary_err(t, want):
    """The worst of a tensor's three distances to a stored summary: the L2 norm, the sum on the scale of its terms, the first 8 elements"""
    got, want = summary(t).double(), torch.as_tensor(want).double()
    n = torch.as_tensor(t).numel()
    return max(abs(float(got[0]) - float(want[0])) / float(want[0]), abs(float(got[1]) - float(want[1])) / (float(want[0]) * math.sqrt(n)),
               rel(got[2:], want[2:]))


def check_grads_f64(grads, fx, b, tol, params=None):
    """Every gradient of a float64 restatement against the fixture's float64 run at beta `b`: tensors of up to 16384 elements are stored in full
    (<b>/g_f64/), the larger ones as summaries (<b>/gs_f64/)"""
    full = {k[len(b) + 7:]: v for k, v in fx.items() if k.startswith(f"{b}/g_f64/")}
    summ = {k[len(b) + 8:]: v for k, v in fx.items() if k.startswith(f"{b}/gs_f64/")}
    assert set(grads) == set(full) | set(summ) and not set(full) & set(summ), (b, sorted(set(grads) ^ (set(full) | set(summ))))
    assert params is None or set(grads) == set(params), (b, "gradients and parameters")
    for k, g in grads.items():
        assert not summ or (torch.as_tensor(g).numel() <= 16384) == (k in full), (b, k)
        e = rel(g, full[k]) if k in full else summary_err(g, summ[k])
        assert e <= tol, (b, k, e)


def check_traj_f64(steps, fx, tol, keys=("loss", "recon", "kld")):
    """A restated trajectory against the fixture's float64 run: the losses, and each parameter in full (<s>/p_f64/) or as its summary (<s>/ps_f64/)"""
    for s, out, p in steps:
        for k in keys:
            assert rel(out[k], fx[f"{s}/{k}_f64"]) <= tol, (s, k)
        for k, v in p.items():
            e = rel(v, fx[f"{s}/p_f64/{k}"]) if f"{s}/p_f64/{k}" in fx else summary_err(v, fx[f"{s}/ps_f64/{k}"])
            assert e <= tol, (s, k, e)


# ---- the conv families (kinds 11, 17): trunk and decoder of models/vae/conv.py --------------------------------------------------------
def conv_trunk(p, prefix, act, x):
    """conv1 .. conv3 of the network `prefix` on 2x - 1 -> h3 [B, 512] (NCHW-flat; vae/conv.py:59-72, vae/auxconv.py:61-72)"""
    a = ACTS[act]
    hdn = (2 * x - 1).view(-1, 1, 28, 28)
    for i in (1, 2, 3):
        hdn = a(F.conv2d(hdn, p[f"{prefix}conv{i}.weight"], p[f"{prefix}conv{i}.bias"], stride=2, padding=2))
    return hdn.reshape(hdn.size(0), -1)


def conv_decode_logit(p, act, z):
    """Decoder.forward's logits as [R, 784] (vae/conv.py:121-131): ZeroPad2d((0, 1, 0, 1)) after deconv1, the 29 x 29 output cropped to 28 x 28"""
    a = ACTS[act]
    hdn = a(lin(p, "decode.fc.fc", a(lin(p, "decode.fc.layers.0", z)))).view(-1, 32, 4, 4)
    hdn = F.pad(a(F.conv_transpose2d(hdn, p["decode.deconv1.weight"], p["decode.deconv1.bias"], stride=2, padding=2)), (0, 1, 0, 1))
    hdn = a(F.conv_transpose2d(hdn, p["decode.deconv2.weight"], p["decode.deconv2.bias"], stride=2, padding=2))
    logit = F.conv_transpose2d(hdn, p["decode.reparam.logit_fn.weight"], p["decode.reparam.logit_fn.bias"], stride=2, padding=2)
    return logit[:, :, :28, :28].reshape(-1, D28)


def bce_rows(logit, x):
    """-> -log p(x | z) per row, and the logits"""
    return F.binary_cross_entropy_with_logits(logit, x, reduction="none").sum(1), logit


def conv_recon_rows(p, act, x, z):
    return bce_rows(conv_decode_logit(p, act, z), x)


# ---- the residual-conv families (kinds 12, 19): trunk and decoder of models/vae/resconv.py --------------------------------------------
def resconv_trunk(p, prefix, center, x):
    """The weight-normalised encoder trunk `prefix` (encode.enc. of vae/resconv.py:58-68, inp_encode.enc. of vae/auxresconv.py:52-63) -> [B, c_dim]"""
    h = (2 * x - 1 if center else x).view(-1, 1, 28, 28)
    for i, st in zip((0, 2, 4, 6, 8), (2, 1, 2, 1, 2)):
        h = F.elu(O.res_conv(p, f"{prefix}{i}.", h, st, F.elu))
    return F.elu(O.res_linear(p, f"{prefix}11.", h.reshape(h.size(0), 512), True))


def resconv_decode_logit(p, z):
    return O.resconv_decode(None, p, z)


def resconv_tail_logit(p, y14):
    """the decoder's last stage on y14 [R, 14, 14, 16] (NHWC): the x2 upsampling, then decode.dec.17 -> [R, 784]"""
    u = F.interpolate(y14.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    return O.res_conv(p, "decode.dec.17.", u, 1, F.elu).reshape(y14.size(0), D28)


def resconv_recon_rows(p, x, z):
    return bce_rows(resconv_decode_logit(p, z), x)


# ---- the MLP auxiliary family (kinds 14, 15) in float64 numpy, backward by hand ---------------------------------------------------------
def sigmoid(v):
    return 0.5 * (1.0 + np.tanh(0.5 * v))


def softplus(v):
    return np.logaddexp(0.0, v)


# activation -> (f(v), f'(v)) on the pre-activation v
NP_ACT = {"relu": (lambda v: np.maximum(v, 0.0), lambda v: (v > 0).astype(v.dtype)),
          "softplus": (softplus, sigmoid),
          "elu": (lambda v: np.where(v > 0, v, np.expm1(np.minimum(v, 0.0))), lambda v: np.where(v > 0, 1.0, np.exp(np.minimum(v, 0.0)))),
          "tanh": (np.tanh, lambda v: 1.0 - np.tanh(v) ** 2),
          "leaky_relu": (lambda v: np.where(v > 0, v, 0.2 * v), lambda v: np.where(v > 0, 1.0, 0.2)),
          "swish": (lambda v: v * sigmoid(v), lambda v: sigmoid(v) * (1.0 + v * (1.0 - sigmoid(v))))}
SPM = {"softplus": 0.0, "spm10": 10.0, "spm6": 6.0, "spm5": 5.0, "spm4": 4.0, "spm3": 3.0, "spm2": 2.0}


def clip_logvar(code, v):
    """NormalDistribution.clip_logvar (models/reparam.py:17-41) -> (c(v), c'(v))"""
    if code in (None, "none"):
        return v, np.ones_like(v)
    if code == "hard":
        return np.clip(v, -4.0, 2.0), ((v > -4.0) & (v < 2.0)).astype(v.dtype)
    if code in SPM:
        return softplus(v + SPM[code]) - SPM[code], sigmoid(v + SPM[code])
    s = {"tanh": 1.0, "2tanh": 2.0}[code]
    return s * np.tanh(v), s * (1.0 - np.tanh(v) ** 2)


def mlp_names(p, prefix):
    n = len([k for k in p if k.startswith(prefix + "layers.") and k.endswith("weight")])
    return [f"{prefix}layers.{i}" for i in range(n)] + [prefix + "fc"]


def mlp_fwd(p, prefix, hdn, act):
    """models/layers.py MLP(..., use_nonlinearity_output=True): `layers.*` then `fc`, every one followed by the activation -> output, cache"""
    cache = []
    for name in mlp_names(p, prefix):
        pre = lin(p, name, hdn)
        cache.append((name, hdn, pre))
        hdn = NP_ACT[act][0](pre)
    return hdn, cache


def mlp_bwd(p, cache, act, dh, grads):
    """dL/d output -> dL/d input, the layers' gradients into `grads`"""
    for name, inp, pre in reversed(cache):
        dpre = dh * NP_ACT[act][1](pre)
        grads[name + ".weight"], grads[name + ".bias"] = dpre.T @ inp, dpre.sum(0)
        dh = dpre @ p[name + ".weight"]
    return dh


def lin_bwd(p, name, hdn, dout, grads):
    grads[name + ".weight"], grads[name + ".bias"] = dout.T @ hdn, dout.sum(0)
    return dout @ p[name + ".weight"]


def aux_recon_rows(family, p, act, x, z):
    """-log p(x | z) per row -> rows, decoder mean, and what the backward needs"""
    hd, cache = mlp_fwd(p, "decode.main.", z, act)
    if family == "mnist":
        logit = lin(p, "decode.reparam.logit_fn", hd)
        rows = (np.maximum(logit, 0) - logit * x + np.logaddexp(0.0, -np.abs(logit))).sum(1)        # BCE with logits
        return rows, sigmoid(logit), (hd, cache, logit, None)
    mx, lvx = lin(p, "decode.reparam.mean_fn", hd), lin(p, "decode.reparam.logvar_fn", hd)
    return 0.5 * (lvx + (x - mx) ** 2 / np.exp(lvx) + LOG_2PI).sum(1), mx, (hd, cache, mx, lvx)


def aux_forward_backward(p, cfg, x, eps, beta, scale):
    """VAE.forward (vae/auxmnist.py:337-364) and d (scale * loss) / d p in closed form -> dict(mu0, lv0, z, mean, loss, recon, kld), grads;
    cfg = (family, activation, clip code of aux_encode's logvar)"""
    family, act, clip = cfg
    B, D = x.shape
    nd = p["aux_encode.reparam.mean_fn.weight"].shape[0]
    eps0, epsz = eps[:, :nd], eps[:, nd:]
    xs = 2 * x - 1 if family == "mnist" else x
    h0, c0 = mlp_fwd(p, "aux_encode.main.", xs, act)
    mu0, lv0r = lin(p, "aux_encode.reparam.mean_fn", h0), lin(p, "aux_encode.reparam.logvar_fn", h0)
    lv0, dclip = clip_logvar(clip, lv0r)
    z0 = mu0 + np.exp(0.5 * lv0) * eps0
    h, c1 = mlp_fwd(p, "encode.fc.", np.concatenate([xs, z0], 1), act)
    mu, lv = lin(p, "encode.reparam.mean_fn", h), lin(p, "encode.reparam.logvar_fn", h)
    z = mu + np.exp(0.5 * lv) * epsz
    hr, c2 = mlp_fwd(p, "aux_decode.fc.", np.concatenate([xs, z], 1), act)
    mup, lvp = lin(p, "aux_decode.reparam.mean_fn", hr), lin(p, "aux_decode.reparam.logvar_fn", hr)
    rec, mean, (hd, c3, o0, o1) = aux_recon_rows(family, p, act, x, z)
    kld, aux = kld_rows(mu, lv), pair_kld_rows(mu0, lv0, mup, lvp)
    out = dict(mu0=mu0, lv0=lv0, z=z, mean=mean, loss=(rec + beta * kld + beta * aux).mean(), recon=rec.mean(), kld=(kld + aux).mean())
    # ---- backward, c = scale / B
    c, g = scale / B, {}
    if family == "mnist":
        dhd = lin_bwd(p, "decode.reparam.logit_fn", hd, c * (sigmoid(o0) - x), g)
    else:
        dhd = lin_bwd(p, "decode.reparam.mean_fn", hd, -c * (x - o0) / np.exp(o1), g)
        dhd = dhd + lin_bwd(p, "decode.reparam.logvar_fn", hd, 0.5 * c * (1 - (x - o0) ** 2 / np.exp(o1)), g)
    dz = mlp_bwd(p, c3, act, dhd, g)
    dmup = c * beta * (mup - mu0) / np.exp(lvp)
    dlvp = c * beta * 0.5 * (1 - (np.exp(lv0) + (mu0 - mup) ** 2) / np.exp(lvp))
    dhr = lin_bwd(p, "aux_decode.reparam.mean_fn", hr, dmup, g) + lin_bwd(p, "aux_decode.reparam.logvar_fn", hr, dlvp, g)
    dz = dz + mlp_bwd(p, c2, act, dhr, g)[:, D:]
    dmu = dz + c * beta * mu
    dlv = dz * (z - mu) / 2 + c * beta * (np.exp(lv) - 1) / 2
    dh = lin_bwd(p, "encode.reparam.mean_fn", h, dmu, g) + lin_bwd(p, "encode.reparam.logvar_fn", h, dlv, g)
    dz0 = mlp_bwd(p, c1, act, dh, g)[:, D:]
    dmu0 = dz0 + c * beta * (mu0 - mup) / np.exp(lvp)
    dlv0 = dz0 * (z0 - mu0) / 2 + c * beta * 0.5 * (np.exp(lv0) / np.exp(lvp) - 1)
    dh0 = lin_bwd(p, "aux_encode.reparam.mean_fn", h0, dmu0, g) + lin_bwd(p, "aux_encode.reparam.logvar_fn", h0, dlv0 * dclip, g)
    mlp_bwd(p, c0, act, dh0, g)
    return out, g


def aux_logq_rows(p, cfg, x, eps):
    """The three stochastic stages of VAE.logprob (vae/auxmnist.py:381-451, sample_size2 = 1) on injected draws eps [B, k, noise + z]
    -> z [B k, zd], logq [B k] = log q(z0|x) + log q(z|z0,x) - log r(z0|z,x)"""
    family, act, clip = cfg
    B, k, _ = eps.shape
    nd = p["aux_encode.reparam.mean_fn.weight"].shape[0]
    xs = 2 * x - 1 if family == "mnist" else x
    h0, _ = mlp_fwd(p, "aux_encode.main.", xs, act)
    mu0 = lin(p, "aux_encode.reparam.mean_fn", h0)
    lv0, _ = clip_logvar(clip, lin(p, "aux_encode.reparam.logvar_fn", h0))
    mu0, lv0, xr = (np.repeat(v, k, 0) for v in (mu0, lv0, xs))
    e = eps.reshape(B * k, -1)
    z0 = mu0 + np.exp(0.5 * lv0) * e[:, :nd]
    h, _ = mlp_fwd(p, "encode.fc.", np.concatenate([xr, z0], 1), act)
    mu, lv = lin(p, "encode.reparam.mean_fn", h), lin(p, "encode.reparam.logvar_fn", h)
    z = mu + np.exp(0.5 * lv) * e[:, nd:]
    hr, _ = mlp_fwd(p, "aux_decode.fc.", np.concatenate([xr, z], 1), act)
    mup, lvp = lin(p, "aux_decode.reparam.mean_fn", hr), lin(p, "aux_decode.reparam.logvar_fn", hr)
    return z, log_normal_rows(z0, mu0, lv0) + log_normal_rows(z, mu, lv) - log_normal_rows(z0, mup, lvp)


def aux_logprob_rows(p, cfg, x, eps):
    """VAE.logprob before its mean, [B]"""
    B, k, _ = eps.shape
    z, logq = aux_logq_rows(p, cfg, x, eps)
    rec, _, _ = aux_recon_rows(cfg[0], p, cfg[1], np.repeat(x, k, 0), z)
    return iw_logsumexp((-rec + log_normal_rows(z, 0.0, 0.0) - logq).reshape(B, k))
