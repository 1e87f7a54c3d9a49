// The conv models (ardae_model_desc.kind 2: ConvIPVAE `--model mnist-conv`; 4: MNISTConvAuxIPVAE `--model auxconv`, noise
// [R, noise_dim + z_dim], hidden context [B, 1600]); csrc/model.hip dispatches to the families.  The conv trunk and the decoder of
// models/vae/conv.py are declared here for the family that shares them (csrc/convvae.hip, kind 11).
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family CONV_FAMILY, AUXCONV_FAMILY;

constexpr int EH[4] = {28, 14, 7, 4};      // encoder spatial sizes
constexpr int ECH[4] = {1, 16, 32, 32};    // encoder channels
// wgrad_splits hint of the conv backward: a tuning value, not the problem count (kinds 2 / 11 push 14)
constexpr int CONV_WGRAD_HINT = 18;

// a Lin's weight is viewed as [out, in] (convs: [O, C*25]; deconvs: [in_ch, out_ch*25], with out_ch bias entries)
struct ConvLayout {
  int nd, zd, act;
  Lin conv[3], fc4, fc5, dfc[2], dcv[3];
  size_t total;
  ConvLayout() : nd(0), zd(0), act(0), total(0) {}     // decoder-only view filled by AuxConvLayout / ConvVaeLayout
  explicit ConvLayout(const ardae_model_desc& d) : nd(d.noise_dim), zd(d.z_dim), act(d.act) {
    size_t off = 0;
    auto add = [&](Lin& l, int out, int in, int nbias) { l = next_lin(off, out, in, nbias); };
    add(conv[0], 16, 1 * 25, 16); add(conv[1], 32, 16 * 25, 32); add(conv[2], 32, 32 * 25, 32);
    add(fc4, 800, 512 + nd, 800); add(fc5, zd, 800, zd);
    decoder(off);
    total = off;
  }
  // the decoder's five operators at parameter offset `off` (advanced past them): decode.fc.{layers.0, fc}, deconv1, deconv2, reparam.logit_fn
  void decoder(size_t& off) {
    dfc[0] = next_lin(off, 300, zd, 300); dfc[1] = next_lin(off, 512, 300, 512);
    dcv[0] = next_lin(off, 32, 32 * 25, 32); dcv[1] = next_lin(off, 32, 16 * 25, 16); dcv[2] = next_lin(off, 16, 1 * 25, 1);
  }
};

struct ConvPacked {
  size_t conv_f[3], conv_b[3], fc4i_f, fc4i_b, fc4n_f, fc5_f, fc5_b, dfc_f[2], dfc_b[2], dcv_f[3], dcv_b[3];
  ConvPacked() {}     // decoder-only view filled by AuxConvPacked / ConvVaePacked
  ConvPacked(const ConvLayout& P, PackList& pl) {
    for (int i = 0; i < 3; ++i) pl.pair(P.conv[i], conv_f[i], conv_b[i]);
    pl.pair(P.fc4, fc4i_f, fc4i_b, 0, 512);                            // [800, 512 + nd]: image half both ways, noise half forward
    fc4n_f = pl.panel(P.fc4.w + 512, P.fc4.in, 800, P.nd, false);
    pl.pair(P.fc5, fc5_f, fc5_b);
    decoder_panels(P, pl);
  }
  explicit ConvPacked(const ConvLayout& P, PackList&& sizing = PackList()) : ConvPacked(P, sizing) {}   // offsets only
  // the decoder's five operators (shared with the hierarchical conv model and the conv baseline, which reserve them at their own offsets)
  void decoder_panels(const ConvLayout& P, PackList& pl) {
    for (int i = 0; i < 2; ++i) pl.pair(P.dfc[i], dfc_f[i], dfc_b[i]);
    for (int i = 0; i < 3; ++i) {   // ConvTranspose2d weight [in, out*25]: forward = X . W (transposed pack), backward-data = dC . W^T (natural)
      dcv_f[i] = pl.panel(P.dcv[i].w, P.dcv[i].in, P.dcv[i].in, P.dcv[i].out, true);
      dcv_b[i] = pl.panel(P.dcv[i].w, P.dcv[i].in, P.dcv[i].out, P.dcv[i].in, false);
    }
  }
};

// spatial sizes: encoder 28 -> 14 -> 7 -> 4; decoder grids 4 -> 8 (7 valid) -> 15 -> 28 (of 29)
struct ConvWs {
  // encoder (B rows)
  float *x2, *cols[3], *hcv[3], *inp, *rb, *t1, *z;
  // decoder (R rows)
  float *d1, *d2, *g0, *c1, *u1, *c2, *u2, *c3, *logit, *rec_row, *pri_row;
  // backward
  float *dlogit, *dc3, *dp2, *dc2, *dp1, *dc1, *dg0, *dd2, *dd1, *dzq, *dz, *dt1, *drb, *dinp, *dinp_t, *dh3, *dcols3, *dh2, *dcols2, *dh1, *ones;
};

// the trunk's forward buffers on B images: x2, cols / hcv of the three convs, inp
void conv_trunk_carve(Bump& ws, size_t B, ConvWs& W);
// the decoder's buffers on R rows of z: forward (d1 .. pri_row), and unless decode_only the backward's (dlogit .. dd1, dzq, dz, ones)
void conv_decoder_carve(Bump& ws, size_t R, int zd, bool decode_only, ConvWs& W);

// conv trunk 1 -> 16 -> 32 -> 32 (k5 s2 p2, 28 -> 14 -> 7 -> 4) on the rescaled images x2 [B, 784]: fills cols / hcv and the
// NCHW-flattened output inp [B, 512]
// (cols0_ready: cols[0], the im2col rows of x2, were filled by an earlier trunk on the same x2 - the three trunks of kind 17 share them)
int trunk_fwd(const Lin* conv, const size_t* conv_f, const float* params, const float* packed, const float* x2, float* const* cols,
              float* const* hcv, float* inp, int B, int act, hipStream_t st, bool cols0_ready = false);
// backward of the trunk from d(inp) [B, 512] (NCHW-flat): dh3 / dh2 / dh1 = d(pre-activation) of conv3 / conv2 / conv1 (NHWC rows)
int trunk_bwd(const size_t* conv_b, const float* packed, const float* dinp, float* dinp_t, float* const* hcv, float* dh3, float* dcols3,
              float* dh2, float* dcols2, float* dh1, int B, int act, hipStream_t st);
// the trunk's three weight-gradient problems (conv3, conv2, conv1) from dh3 / dh2 / dh1 and the saved im2col rows
void conv_trunk_wgrads(const Lin* conv, float* const* cols, const float* dh3, const float* dh2, const float* dh1, int B, WgradList& wl);
// models/vae/conv.py::Decoder on R rows of z (P, K: the dfc / dcv members): fills W.d1 .. W.logit [R, 784]
int conv_decode_fwd(const ConvLayout& P, const ConvPacked& K, const float* params, const float* packed, const float* z, int R, ConvWs& W,
                    hipStream_t st);
// its two halves: up to W.u1 [R, 8, 8, 32] (decode.fc, deconv1 with its activation and zero pad: fills W.d1, d2, g0, c1, u1), and the last two stages
// from u1 as the four unfused launches (deconv2, logit_fn)
int conv_decode_head_fwd(const ConvLayout& P, const ConvPacked& K, const float* params, const float* packed, const float* z, int R, ConvWs& W,
                         hipStream_t st);
int conv_decode_tail_fwd(const ConvLayout& P, const ConvPacked& K, const float* params, const float* packed, const float* u1, int R, float* c2, float* u2,
                         float* c3, float* logit, hipStream_t st);
// the same two stages as ONE launch (conv_tail_kernel, csrc/convmodel.hip): u1 [R, 8, 8, 32] -> logit [R, 784]; b2 / b3: the biases of decode.deconv2 and
// decode.reparam.logit_fn in the parameter buffer, wt2 [CT_W2] / wt3 [CT_W3]: their weights (ConvTranspose2d layout [in, out, 5, 5]) as
// launch_conv_tail_pack re-lays them, on 16-byte boundaries of the packed buffer
constexpr size_t CT_W2 = 32 * 25 * 16, CT_W3 = 16 * 32;
int launch_conv_tail(const float* u1, const float* wt2, const float* b2, const float* wt3, const float* b3, int R, int act, float* logit, hipStream_t st);
int launch_conv_tail_pack(const float* w2, const float* w3, float* wt2, float* wt3, hipStream_t st);
// decoder backward from W.dlogit (and W.dzq = the part of dL/dz that does not pass through the decoder): fills dc3 / dp2 / dc2 / dp1 / dc1 / dg0 /
// dd2 / dd1 and W.dz
int conv_decoder_bwd(const ConvLayout& P, const ConvPacked& K, const float* packed, ConvWs& W, int R, hipStream_t st);
// the decoder's eight weight-gradient problems (z: W.z)
void conv_decoder_wgrads(const ConvLayout& P, const ConvWs& W, int R, WgradList& wl);
}  // namespace ardae
