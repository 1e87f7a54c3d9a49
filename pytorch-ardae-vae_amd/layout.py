"""Parameter names / shapes / flat-buffer offsets, identical to the reference's `named_parameters()` order.

Reference: models/layers.py:477-515 (MLP: `layers.{i}.{weight,bias}`, `fc.{weight,bias}`), :681-724 (ContextConcatMLP),
models/ivae/mnist.py:123-199, models/ivae/toy.py:154-194,694-737, models/graddae/mlp.py:57,137,342-378,
models/resdae/mlp.py:45,111,287-326.  The C++ side (csrc/cdae.hip, csrc/model.hip) computes the same offsets; the ABI
test checks `ardae_*_param_floats` against these totals.
"""
import math


def _mlp(prefix, din, dh, dout, n_hidden, extra_in=0):
    spec = []
    for i in range(n_hidden):
        spec += [(f"{prefix}layers.{i}.weight", (dh, (din if i == 0 else dh) + extra_in)), (f"{prefix}layers.{i}.bias", (dh,))]
    spec += [(f"{prefix}fc.weight", (dout, (din if n_hidden == 0 else dh) + extra_in)), (f"{prefix}fc.bias", (dout,))]
    return spec


def _res_block(prefix, out, inn, conv):
    """A weight-normalised residual block (models/layers2.py:50-93,237-352; models/layers.py:25-85 inside ResMLP): three operators, each with
    direction / scale / bias."""
    def wn(pre):
        o_in = out if pre.endswith("h1.") else inn
        return [(pre + "direction", (out, o_in, 3, 3) if conv else (out, o_in)), (pre + "scale", (out,)), (pre + "bias", (out,))]
    a, b, c = ("conv_0h.", "conv_h1.", "conv_01.") if conv else ("dot_0h.", "dot_h1.", "dot_01.")
    return wn(prefix + a) + wn(prefix + b) + wn(prefix + c)


def _resconv_trunk(tp, cdim):
    """ResConv2d 1 -> 16 s2, 16 -> 16, 16 -> 32 s2, 32 -> 32, 32 -> 32 s2, then ResLinear(512 -> c_dim) under the prefix `tp`"""
    s = []
    for i, (o, inn) in zip((0, 2, 4, 6, 8), ((16, 1), (16, 16), (32, 16), (32, 32), (32, 32))):
        s += _res_block(f"{tp}{i}.", o, inn, True)
    return s + _res_block(f"{tp}11.", cdim, 512, False)


def _resconv_decoder(z_dim, cdim):
    """models/vae/resconv.py:87-106: two ResLinears, five ResConv2d"""
    s = _res_block("decode.dec.0.", cdim, z_dim, False) + _res_block("decode.dec.2.", 512, cdim, False)
    for i, (o, inn) in zip((6, 8, 12, 14, 17), ((32, 32), (32, 32), (16, 32), (16, 16), (1, 16))):
        s += _res_block(f"decode.dec.{i}.", o, inn, True)
    return s


def model_spec(kind, input_dim, noise_dim, h_dim, z_dim, n_layers, enc_type="res-wn-mlp"):
    if kind == "mnist":
        s = _mlp("encode.inp_encode.", input_dim, h_dim, h_dim, n_layers + 1)
        s += _mlp("encode.fc.", h_dim + noise_dim, h_dim, z_dim, 1)
        s += _mlp("decode.main.", z_dim, h_dim, h_dim, n_layers)
        s += [("decode.reparam.logit_fn.weight", (input_dim, h_dim)), ("decode.reparam.logit_fn.bias", (input_dim,))]
    elif kind == "conv":   # models/ivae/conv.py:44-136 + models/vae/conv.py:79-136 (28x28x1, fixed architecture)
        s = [("encode.conv1.weight", (16, 1, 5, 5)), ("encode.conv1.bias", (16,)),
             ("encode.conv2.weight", (32, 16, 5, 5)), ("encode.conv2.bias", (32,)),
             ("encode.conv3.weight", (32, 32, 5, 5)), ("encode.conv3.bias", (32,)),
             ("encode.fc4.weight", (800, 512 + noise_dim)), ("encode.fc4.bias", (800,)),
             ("encode.fc5.weight", (z_dim, 800)), ("encode.fc5.bias", (z_dim,))]
        s += _mlp("decode.fc.", z_dim, 300, 512, 1)
        s += [("decode.deconv1.weight", (32, 32, 5, 5)), ("decode.deconv1.bias", (32,)),
              ("decode.deconv2.weight", (32, 16, 5, 5)), ("decode.deconv2.bias", (16,)),
              ("decode.reparam.logit_fn.weight", (16, 1, 5, 5)), ("decode.reparam.logit_fn.bias", (1,))]
    elif kind in ("resconv", "auxresconv"):
        # weight-normalised residual blocks (_res_block): ivae/resconv.py:81-125, vae/auxresconv.py:36-63,94,149-153, vae/resconv.py:89-109
        cdim = 512 if kind == "resconv" else h_dim
        s = _resconv_trunk("encode.inp_encode." if kind == "resconv" else "encode.inp_encode.enc.", cdim)
        if kind == "resconv":
            s += resconv_head_spec(enc_type, n_layers, cdim + noise_dim, h_dim, z_dim)
        else:
            s += [("encode.aux_encode.reparam.mean_fn.weight", (noise_dim, cdim)), ("encode.aux_encode.reparam.mean_fn.bias", (noise_dim,)),
                  ("encode.aux_encode.reparam.logvar_fn.weight", (noise_dim, cdim)), ("encode.aux_encode.reparam.logvar_fn.bias", (noise_dim,)),
                  ("encode.encode.fc.0.weight", (cdim, cdim + noise_dim)), ("encode.encode.fc.0.bias", (cdim,)),
                  ("encode.encode.reparam.mean_fn.weight", (z_dim, cdim)), ("encode.encode.reparam.mean_fn.bias", (z_dim,)),
                  ("encode.encode.reparam.logvar_fn.weight", (z_dim, cdim)), ("encode.encode.reparam.logvar_fn.bias", (z_dim,))]
        s += _resconv_decoder(z_dim, cdim)
    elif kind == "toy":
        s = _mlp("encode.inp_encode.", input_dim, h_dim, h_dim, n_layers - 1)
        s += _mlp("encode.fc.", h_dim, h_dim, z_dim, n_layers, extra_in=noise_dim)
        s += _mlp("decode.main.", z_dim, h_dim, h_dim, n_layers - 1)
        s += [("decode.reparam.mean_fn.weight", (input_dim, h_dim)), ("decode.reparam.mean_fn.bias", (input_dim,)),
              ("decode.reparam.logvar_fn.weight", (input_dim, h_dim)), ("decode.reparam.logvar_fn.bias", (input_dim,))]
    elif kind == "auxtoy":     # models/ivae/auxtoy.py:44-130 (AuxEncoder + SimpleEncoder of models/vae/auxtoy.py) + models/vae/toy.py Decoder (Gaussian)
        s = _mlp("encode.aux_encode.main.", input_dim, h_dim, h_dim, n_layers - 1)
        s += [("encode.aux_encode.reparam.mean_fn.weight", (noise_dim, h_dim)), ("encode.aux_encode.reparam.mean_fn.bias", (noise_dim,)),
              ("encode.aux_encode.reparam.logvar_fn.weight", (noise_dim, h_dim)), ("encode.aux_encode.reparam.logvar_fn.bias", (noise_dim,))]
        s += _mlp("encode.encode.fc.", input_dim + noise_dim, h_dim, h_dim, n_layers - 1)
        s += [("encode.encode.reparam.mean_fn.weight", (z_dim, h_dim)), ("encode.encode.reparam.mean_fn.bias", (z_dim,)),
              ("encode.encode.reparam.logvar_fn.weight", (z_dim, h_dim)), ("encode.encode.reparam.logvar_fn.bias", (z_dim,))]
        s += _mlp("decode.main.", z_dim, h_dim, h_dim, n_layers - 1)
        s += [("decode.reparam.mean_fn.weight", (input_dim, h_dim)), ("decode.reparam.mean_fn.bias", (input_dim,)),
              ("decode.reparam.logvar_fn.weight", (input_dim, h_dim)), ("decode.reparam.logvar_fn.bias", (input_dim,))]
    elif kind == "auxmnist":   # models/ivae/auxmnist.py:47-132 (AuxEncoder + SimpleEncoder of models/vae/auxmnist.py) + models/vae/mnist.py Decoder
        s = _mlp("encode.aux_encode.main.", input_dim, h_dim, h_dim, n_layers - 1)
        s += [("encode.aux_encode.reparam.mean_fn.weight", (noise_dim, h_dim)), ("encode.aux_encode.reparam.mean_fn.bias", (noise_dim,)),
              ("encode.aux_encode.reparam.logvar_fn.weight", (noise_dim, h_dim)), ("encode.aux_encode.reparam.logvar_fn.bias", (noise_dim,))]
        s += _mlp("encode.encode.fc.", input_dim + noise_dim, h_dim, h_dim, n_layers - 1)
        s += [("encode.encode.reparam.mean_fn.weight", (z_dim, h_dim)), ("encode.encode.reparam.mean_fn.bias", (z_dim,)),
              ("encode.encode.reparam.logvar_fn.weight", (z_dim, h_dim)), ("encode.encode.reparam.logvar_fn.bias", (z_dim,))]
        s += _mlp("decode.main.", z_dim, h_dim, h_dim, n_layers - 1)
        s += [("decode.reparam.logit_fn.weight", (input_dim, h_dim)), ("decode.reparam.logit_fn.bias", (input_dim,))]
    elif kind == "auxconv":    # models/ivae/auxconv.py:48-126 (AuxEncoder + Encoder of models/vae/auxconv.py) + models/vae/conv.py Decoder
        def trunk(prefix, fc_in):
            return [(prefix + "conv1.weight", (16, 1, 5, 5)), (prefix + "conv1.bias", (16,)),
                    (prefix + "conv2.weight", (32, 16, 5, 5)), (prefix + "conv2.bias", (32,)),
                    (prefix + "conv3.weight", (32, 32, 5, 5)), (prefix + "conv3.bias", (32,)),
                    (prefix + "fc.weight", (800, fc_in)), (prefix + "fc.bias", (800,))]
        def heads(prefix, out):
            return [(prefix + "reparam.mean_fn.weight", (out, 800)), (prefix + "reparam.mean_fn.bias", (out,)),
                    (prefix + "reparam.logvar_fn.weight", (out, 800)), (prefix + "reparam.logvar_fn.bias", (out,))]
        s = trunk("encode.aux_encode.", 512) + heads("encode.aux_encode.", noise_dim)
        s += trunk("encode.encode.", 512 + noise_dim) + heads("encode.encode.", z_dim)
        s += _mlp("decode.fc.", z_dim, 300, 512, 1)
        s += [("decode.deconv1.weight", (32, 32, 5, 5)), ("decode.deconv1.bias", (32,)),
              ("decode.deconv2.weight", (32, 16, 5, 5)), ("decode.deconv2.bias", (16,)),
              ("decode.reparam.logit_fn.weight", (16, 1, 5, 5)), ("decode.reparam.logit_fn.bias", (1,))]
    else:
        raise NotImplementedError(kind)
    return s


def vae_spec(kind, input_dim, h_dim, z_dim, n_layers):
    """The Gaussian-posterior baselines of vae.py (models/vae/mnist.py:28-122 'mnist', models/vae/toy.py:21-120 'toy'): encoder and decoder are
    MLP(..., num_hidden_layers - 1, use_nonlinearity_output=True) - n_layers Linear -> act each - with NormalDistributionLinear /
    BernoulliDistributionLinear heads.  ardae_model_desc.kind 8 ('mnist') / 9 ('toy')."""
    if kind not in ("mnist", "toy"):
        raise NotImplementedError(kind)
    s = _mlp("encode.main.", input_dim, h_dim, h_dim, n_layers - 1)
    s += [("encode.reparam.mean_fn.weight", (z_dim, h_dim)), ("encode.reparam.mean_fn.bias", (z_dim,)),
          ("encode.reparam.logvar_fn.weight", (z_dim, h_dim)), ("encode.reparam.logvar_fn.bias", (z_dim,))]
    s += _mlp("decode.main.", z_dim, h_dim, h_dim, n_layers - 1)
    if kind == "mnist":
        return s + [("decode.reparam.logit_fn.weight", (input_dim, h_dim)), ("decode.reparam.logit_fn.bias", (input_dim,))]
    return s + [("decode.reparam.mean_fn.weight", (input_dim, h_dim)), ("decode.reparam.mean_fn.bias", (input_dim,)),
                ("decode.reparam.logvar_fn.weight", (input_dim, h_dim)), ("decode.reparam.logvar_fn.bias", (input_dim,))]


def aux_vae_spec(kind, input_dim, noise_dim, h_dim, z_dim, n_layers):
    """The auxiliary-variable Gaussian baselines of vae.py (models/vae/auxmnist.py:268-311 'mnist', models/vae/auxtoy.py 'toy'): AuxEncoder (an MLP and a
    NormalDistributionLinear head on z0), SimpleEncoder (`fc` on cat[x, z0], a head on z), the decoder of 'mnist' / 'toy' above and AuxDecoder (`fc` on
    cat[x, z], a head on z0), in the order the reference assigns them; inp_encode / nos_encode / ltt_encode are Identity and own nothing.
    ardae_model_desc.kind 14 ('mnist') / 15 ('toy')."""
    if kind not in ("mnist", "toy"):
        raise NotImplementedError(kind)

    def head(prefix, out):
        return [(prefix + "mean_fn.weight", (out, h_dim)), (prefix + "mean_fn.bias", (out,)),
                (prefix + "logvar_fn.weight", (out, h_dim)), (prefix + "logvar_fn.bias", (out,))]
    s = _mlp("aux_encode.main.", input_dim, h_dim, h_dim, n_layers - 1) + head("aux_encode.reparam.", noise_dim)
    s += _mlp("encode.fc.", input_dim + noise_dim, h_dim, h_dim, n_layers - 1) + head("encode.reparam.", z_dim)
    s += _mlp("decode.main.", z_dim, h_dim, h_dim, n_layers - 1)
    if kind == "mnist":
        s += [("decode.reparam.logit_fn.weight", (input_dim, h_dim)), ("decode.reparam.logit_fn.bias", (input_dim,))]
    else:
        s += head("decode.reparam.", input_dim)
    return s + _mlp("aux_decode.fc.", input_dim + z_dim, h_dim, h_dim, n_layers - 1) + head("aux_decode.reparam.", noise_dim)


def conv_vae_spec(z_dim):
    """The conv Gaussian-posterior baseline of vae.py (models/vae/conv.py:29-168, `--model conv`; 28 x 28 x 1, fixed architecture): the conv
    trunk of the 'conv' implicit model, `encode.fc` 512 -> 800, a NormalDistributionLinear head and that model's decoder.  ardae_model_desc.kind 11."""
    s = [("encode.conv1.weight", (16, 1, 5, 5)), ("encode.conv1.bias", (16,)),
         ("encode.conv2.weight", (32, 16, 5, 5)), ("encode.conv2.bias", (32,)),
         ("encode.conv3.weight", (32, 32, 5, 5)), ("encode.conv3.bias", (32,)),
         ("encode.fc.weight", (800, 512)), ("encode.fc.bias", (800,)),
         ("encode.reparam.mean_fn.weight", (z_dim, 800)), ("encode.reparam.mean_fn.bias", (z_dim,)),
         ("encode.reparam.logvar_fn.weight", (z_dim, 800)), ("encode.reparam.logvar_fn.bias", (z_dim,))]
    s += _mlp("decode.fc.", z_dim, 300, 512, 1)
    return s + [("decode.deconv1.weight", (32, 32, 5, 5)), ("decode.deconv1.bias", (32,)),
                ("decode.deconv2.weight", (32, 16, 5, 5)), ("decode.deconv2.bias", (16,)),
                ("decode.reparam.logit_fn.weight", (16, 1, 5, 5)), ("decode.reparam.logit_fn.bias", (1,))]


def aux_conv_vae_spec(noise_dim, z_dim):
    """The hierarchical conv Gaussian baseline of vae.py (models/vae/auxconv.py, `--model auxconv`; 28 x 28 x 1, fixed architecture): AuxEncoder (a conv
    trunk, `fc` 512 -> 800, a NormalDistributionLinear head on z0 of width noise_dim), Encoder (its own trunk, `fc` on cat[h3, z0], a head on z), the
    decoder of conv_vae_spec and AuxDecoder (its own trunk, `fc` on cat[h3, z], a head on z0), in the order the reference assigns them.
    ardae_model_desc.kind 17."""
    def net(prefix, extra, out):
        return [(prefix + "conv1.weight", (16, 1, 5, 5)), (prefix + "conv1.bias", (16,)),
                (prefix + "conv2.weight", (32, 16, 5, 5)), (prefix + "conv2.bias", (32,)),
                (prefix + "conv3.weight", (32, 32, 5, 5)), (prefix + "conv3.bias", (32,)),
                (prefix + "fc.weight", (800, 512 + extra)), (prefix + "fc.bias", (800,)),
                (prefix + "reparam.mean_fn.weight", (out, 800)), (prefix + "reparam.mean_fn.bias", (out,)),
                (prefix + "reparam.logvar_fn.weight", (out, 800)), (prefix + "reparam.logvar_fn.bias", (out,))]
    decoder = [(n, s) for n, s in conv_vae_spec(z_dim) if n.startswith("decode.")]
    return net("aux_encode.", 0, noise_dim) + net("encode.", noise_dim, z_dim) + decoder + net("aux_decode.", z_dim, noise_dim)


def resconv_vae_spec(z_dim, c_dim):
    """The residual-conv Gaussian-posterior baseline of vae.py (models/vae/resconv.py:26-148, `--model resconv`; 28 x 28 x 1): the weight-normalised
    trunk of the 'auxresconv' implicit model as `encode.enc.*` (width c_dim), a NormalDistributionLinear head and that model's decoder.
    ardae_model_desc.kind 12."""
    return (_resconv_trunk("encode.enc.", c_dim)
            + [("encode.reparam.mean_fn.weight", (z_dim, c_dim)), ("encode.reparam.mean_fn.bias", (z_dim,)),
               ("encode.reparam.logvar_fn.weight", (z_dim, c_dim)), ("encode.reparam.logvar_fn.bias", (z_dim,))]
            + _resconv_decoder(z_dim, c_dim))


def aux_resconv_vae_spec(noise_dim, z_dim, c_dim):
    """The hierarchical residual-conv Gaussian baseline of vae.py (models/vae/auxresconv.py:254-284, `--model auxresconv` / `auxresconvct`; 28 x 28 x 1):
    ONE weight-normalised trunk `inp_encode.enc.*` (width c_dim), AuxEncoder (a NormalDistributionLinear head on z0 of width noise_dim), Encoder
    (`fc.0` on cat[ctx, z0], a head on z), the decoder of resconv_vae_spec and AuxDecoder (`fc.0` on cat[ctx, z], a head on z0), in the order the
    reference assigns them.  ardae_model_desc.kind 19."""
    def head(prefix, out):
        return [(prefix + "reparam.mean_fn.weight", (out, c_dim)), (prefix + "reparam.mean_fn.bias", (out,)),
                (prefix + "reparam.logvar_fn.weight", (out, c_dim)), (prefix + "reparam.logvar_fn.bias", (out,))]

    def fc(prefix, extra):
        return [(prefix + "fc.0.weight", (c_dim, c_dim + extra)), (prefix + "fc.0.bias", (c_dim,))]
    return (_resconv_trunk("inp_encode.enc.", c_dim) + head("aux_encode.", noise_dim) + fc("encode.", noise_dim) + head("encode.", z_dim)
            + _resconv_decoder(z_dim, c_dim) + fc("aux_decode.", z_dim) + head("aux_decode.", noise_dim))


def cdae_spec(kind, input_dim, context_dim, h_dim, n_layers, enc_input=True):
    """The conditional AR-DAE (models/graddae/mlp.py:342-378, models/resdae/mlp.py:287-326): `layers.0.weight` of the last MLP is [h, 2h + 1] =
    [W1a | W1c | w1s] (ardae_cdae_desc.kind 0 'grad' / 1 'res').  enc_input=False: there is no inp_encode and the last MLP reads x_bar itself,
    [h, d + h + 1] = [W1x | W1c | w1s] (kind 16 / 17)."""
    s = _mlp("ctx_encode.", context_dim, h_dim, h_dim, n_layers - 1)
    if enc_input:
        s += _mlp("inp_encode.", input_dim, h_dim, h_dim, n_layers - 1)
    first = (h_dim if enc_input else input_dim) + h_dim + 1
    if kind == "grad":
        s += _mlp("neglogprob.", first, h_dim, 1, n_layers)
    elif kind == "res":
        s += _mlp("dae.", first, h_dim, input_dim, n_layers)
    else:
        raise NotImplementedError(kind)
    return s


def cdae_plain_spec(kind, input_dim, context_dim, h_dim, n_layers):
    """The plain conditional DAE (models/graddae/mlp.py:243-247, models/resdae/mlp.py:203-207): cdae_spec without the sigma column,
    `layers.0.weight` is [h, 2h] = [W1a | W1c].  ardae_cdae_desc.kind 10 ('grad') / 11 ('res')."""
    s = _mlp("ctx_encode.", context_dim, h_dim, h_dim, n_layers - 1)
    s += _mlp("inp_encode.", input_dim, h_dim, h_dim, n_layers - 1)
    if kind == "grad":
        return s + _mlp("neglogprob.", 2 * h_dim, h_dim, 1, n_layers)
    if kind == "res":
        return s + _mlp("dae.", 2 * h_dim, h_dim, input_dim, n_layers)
    raise NotImplementedError(kind)


def recon_cdae_spec(input_dim, context_dim, h_dim, n_layers, enc_input):
    """The reconstruction conditional DAE (models/dae/mlp.py:116-120, enc_ctx=True): ctx_encode.*, inp_encode.* (enc_input only), dae.*.
    enc_input=True is cdae_plain_spec('res', ...) (ardae_cdae_desc.kind 11); enc_input=False (the reference's default) has no input encoder and
    `dae.layers.0.weight` is [h, d + h] = [W1x | W1c] (kind 13).  With n_layers = 1 each encoder is a single `fc`."""
    if enc_input:
        return cdae_plain_spec("res", input_dim, context_dim, h_dim, n_layers)
    return _mlp("ctx_encode.", context_dim, h_dim, h_dim, n_layers - 1) + _mlp("dae.", input_dim + h_dim, h_dim, input_dim, n_layers)


def dae_spec(kind, input_dim, h_dim, n_layers):
    """The unconditional AR-DAE (models/graddae/mlp.py:137, models/resdae/mlp.py:111): one MLP on [x_bar | sigma]; `layers.0.weight`
    is [h, d + 1] = [W1x | w1s].  ardae_cdae_desc.kind 2 ('grad') / 3 ('res')."""
    if kind == "grad":
        return _mlp("neglogprob.", input_dim + 1, h_dim, 1, n_layers)
    if kind == "res":
        return _mlp("main.", input_dim + 1, h_dim, input_dim, n_layers)
    raise NotImplementedError(kind)


def dae_plain_spec(kind, input_dim, h_dim, n_layers):
    """The plain DAE of notebooks/dae_toy.ipynb (models/graddae/mlp.py:57, models/resdae/mlp.py:45): one MLP on x_bar alone;
    `layers.0.weight` is [h, d], there is no sigma column.  ardae_cdae_desc.kind 6 ('grad') / 7 ('res')."""
    if kind == "grad":
        return _mlp("neglogprob.", input_dim, h_dim, 1, n_layers)
    if kind == "res":
        return _mlp("main.", input_dim, h_dim, input_dim, n_layers)
    raise NotImplementedError(kind)


def gen_spec(input_dim, hidden_dim, z_dim, n_layers):
    """The implicit generator of notebooks/ardae_fit.ipynb: `main = nn.Sequential(Linear, act, Linear, act, ..., Linear)` - the Linears sit
    at the even indices, main.{0, 2, ..., 2 n_layers}."""
    s = []
    for i in range(n_layers):
        s += [(f"main.{2 * i}.weight", (hidden_dim, z_dim if i == 0 else hidden_dim)), (f"main.{2 * i}.bias", (hidden_dim,))]
    return s + [(f"main.{2 * n_layers}.weight", (input_dim, hidden_dim)), (f"main.{2 * n_layers}.bias", (input_dim,))]


def offsets(spec):
    out, off = {}, 0
    for name, shape in spec:
        n = math.prod(shape)
        out[name] = (off, n, shape)
        off += n
    return out, off


RESCONV_HEADS = {"res-wn-mlp": 0, "mlp": 1, "res-mlp": 2, "res-wn-mlp-lin": 3, "res-mlp-lin": 4}     # ardae_model_desc.flags bits 1-3


def resconv_head_spec(enc_type, n_layers, cin, h_dim, z_dim):
    """Parameters of ResConvIPVAE's sampler head `encode.fc` in the reference's order (models/ivae/resconv.py:101-116): an MLP
    ('mlp'), a ResMLP of ResLinear blocks ('res-wn-mlp': un-normalised WeightNormalizedLinear operators direction / scale / bias;
    'res-mlp': nn.Linear operators weight / bias; models/layers.py:25-85,477-515,559-622) or `Sequential(ResMLP(... -> h_dim, output
    activated), Linear(h_dim, z_dim))` ('-lin').  A ResLinear whose input and output widths coincide has no skip operator (same_dim)."""
    if enc_type not in RESCONV_HEADS:
        raise AssertionError(enc_type)                      # ivae/resconv.py:77
    lin = lambda pre, out, inn: [(pre + "weight", (out, inn)), (pre + "bias", (out,))]

    def oper(pre, out, inn, wn):
        return [(pre + "direction", (out, inn)), (pre + "scale", (out,)), (pre + "bias", (out,))] if wn else lin(pre, out, inn)

    def res(pre, out, inn, wn):
        return oper(pre + "dot_0h.", out, inn, wn) + oper(pre + "dot_h1.", out, out, wn) + ([] if inn == out else oper(pre + "dot_01.", out, inn, wn))
    s = []
    if enc_type == "mlp":
        for i in range(n_layers):
            s += lin(f"encode.fc.layers.{i}.", h_dim, cin if i == 0 else h_dim)
        return s + lin("encode.fc.fc.", z_dim, h_dim)
    wn = enc_type.startswith("res-wn")
    if enc_type in ("res-wn-mlp", "res-mlp"):
        for i in range(n_layers):
            s += res(f"encode.fc.layers.{i}.", h_dim, cin if i == 0 else h_dim, wn)
        return s + res("encode.fc.fc.", z_dim, h_dim, wn)
    for i in range(n_layers - 1):
        s += res(f"encode.fc.0.layers.{i}.", h_dim, cin if i == 0 else h_dim, wn)
    return s + res("encode.fc.0.fc.", h_dim, cin if n_layers == 1 else h_dim, wn) + lin("encode.fc.1.", z_dim, h_dim)
