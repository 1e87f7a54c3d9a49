// What the four plain-conv kinds of ardae_model_desc are joined from (2: ConvIPVAE `--model mnist-conv`, csrc/convmodel.hip; 4: MNISTConvAuxIPVAE
// `--model auxconv`, csrc/auxconvmodel.hip; 11: MNISTConvVAE, csrc/convvae.hip; 17: MNISTConvAuxVAE, csrc/auxconvvae.hip): ONE conv trunk and ONE
// decoder (models/vae/conv.py), each with its layout walk, its panels, its buffer types and carves and its forward / backward / weight-gradient
// problems, and the rules the two Gaussian kinds share.  A kind holds a trunk's and the decoder's pieces as members, next to its own rows; the kernels
// and the bodies are csrc/convmodel.hip's.  csrc/model.hip dispatches to the families.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family CONV_FAMILY, AUXCONV_FAMILY;

constexpr int EH[4] = {28, 14, 7, 4};      // encoder spatial sizes
constexpr int ECH[4] = {1, 16, 32, 32};    // encoder channels
// wgrad_splits hint of the conv backward: a tuning value, not the problem count (kinds 2 / 11 push 14)
constexpr int CONV_WGRAD_HINT = 18;

// the descriptor rules of kinds 2 / 4
int conv_desc_check(const ardae_model_desc* d);
// the rules kinds 11 and 17 share (input_dim 784, h_dim 800, n_layers 1, z_dim >= 1, any activation but NONE); the messages name d->kind, the class and
// what h_dim is the width of.  Each kind puts its noise_dim and flags rules in front.
int conv_gauss_desc_check(const ardae_model_desc* d, const char* cls, const char* h_dim_of);

// ------------------------------------------------------------------------------------------------ the trunk: conv 1 -> 16 -> 32 -> 32, k5 s2 p2, 28 -> 14 -> 7 -> 4
// a Lin's weight is viewed as [out, in] (convs: [O, C*25]; deconvs: [in_ch, out_ch*25], with out_ch bias entries)
// the trunk's three Lins at parameter offset `off` (advanced past them), and their panel pairs
inline void trunk_lins(size_t& off, Lin* conv) { for (int i = 0; i < 3; ++i) conv[i] = next_lin(off, ECH[i + 1], ECH[i] * 25); }
inline void trunk_panels(const Lin* conv, PackList& pl, size_t* conv_f, size_t* conv_b) { for (int i = 0; i < 3; ++i) pl.pair(conv[i], conv_f[i], conv_b[i]); }
// one trunk's buffers on B images: the im2col rows and the output of each conv, the NCHW-flattened output inp [B, 512]; the backward's d(inp) and
// dh3 / dh2 / dh1 = d(pre-activation) of conv3 / conv2 / conv1 (NHWC rows)
struct TrunkBuf { float *cols[3], *hcv[3], *inp, *dinp, *dh3, *dh2, *dh1; };
// what trunk_bwd reuses from trunk to trunk
struct TrunkScratch { float *dinp_t, *dcols3, *dcols2; };
// T's forward buffers (first: an earlier trunk on the same x2, whose im2col rows of x2 T shares - the three trunks of kind 17 do)
void trunk_carve(Bump& ws, size_t B, TrunkBuf& T, const TrunkBuf* first = nullptr);
// T's backward buffers and, where S is given, a scratch set (first: an earlier set, whose dinp_t S shares)
void trunk_bwd_carve(Bump& ws, size_t B, TrunkBuf& T, TrunkScratch* S, const TrunkScratch* first = nullptr);

// the trunk on the rescaled images x2 [B, 784]: fills T.cols / T.hcv and T.inp (cols0_ready: an earlier trunk on the same x2 filled T.cols[0])
int trunk_fwd(const Lin* conv, const size_t* conv_f, const float* params, const float* packed, const float* x2, const TrunkBuf& T, int B, int act,
              hipStream_t st, bool cols0_ready = false);
// backward of the trunk from T.dinp [B, 512] (NCHW-flat): fills T.dh3 / dh2 / dh1
int trunk_bwd(const size_t* conv_b, const float* packed, const TrunkBuf& T, const TrunkScratch& S, int B, int act, hipStream_t st);
// the trunk's three weight-gradient problems (conv3, conv2, conv1) from dh3 / dh2 / dh1 and the saved im2col rows
void conv_trunk_wgrads(const Lin* conv, const TrunkBuf& T, int B, WgradList& wl);

// ------------------------------------------------------------------------------------------------ the decoder: models/vae/conv.py::Decoder
// its five operators at parameter offset `off` (advanced past them): decode.fc.{layers.0, fc}, deconv1, deconv2, reparam.logit_fn
// (default: all zero, until the owner's walk reaches the decoder)
struct ConvDecLayout {
  int zd = 0, act = 0;
  Lin dfc[2] = {}, dcv[3] = {};
  ConvDecLayout() = default;
  ConvDecLayout(int zd_, int act_, size_t& off) : zd(zd_), act(act_) {
    dfc[0] = next_lin(off, 300, zd, 300); dfc[1] = next_lin(off, 512, 300, 512);
    dcv[0] = next_lin(off, 32, 32 * 25, 32); dcv[1] = next_lin(off, 32, 16 * 25, 16); dcv[2] = next_lin(off, 16, 1 * 25, 1);
  }
};
struct ConvDecPacked {
  size_t dfc_f[2] = {}, dfc_b[2] = {}, dcv_f[3] = {}, dcv_b[3] = {};
  ConvDecPacked() = default;
  ConvDecPacked(const ConvDecLayout& D, PackList& pl) {
    for (int i = 0; i < 2; ++i) pl.pair(D.dfc[i], dfc_f[i], dfc_b[i]);
    for (int i = 0; i < 3; ++i) {   // ConvTranspose2d weight [in, out*25]: forward = X . W (transposed pack), backward-data = dC . W^T (natural)
      dcv_f[i] = pl.panel(D.dcv[i].w, D.dcv[i].in, D.dcv[i].in, D.dcv[i].out, true);
      dcv_b[i] = pl.panel(D.dcv[i].w, D.dcv[i].in, D.dcv[i].out, D.dcv[i].in, false);
    }
  }
};
// its buffers on R rows of z; decoder grids 4 -> 8 (7 valid) -> 15 -> 28 (of 29)
struct ConvDecWs {
  float *d1, *d2, *g0, *c1, *u1, *c2, *u2, *c3, *logit, *rec_row, *pri_row;
  float *dlogit, *dc3, *dp2, *dc2, *dp1, *dc1, *dg0, *dd2, *dd1, *dzq, *dz, *ones;      // backward
};
// which of them a use needs - head: d1 .. u1; tail: c2, u2, c3, logit (the unfused tail's; conv_tail_kernel writes the caller's logits); loss: the
// two loss rows; bwd: dlogit .. ones
struct ConvDecRuns { bool head, tail, loss, bwd; };
constexpr ConvDecRuns CONV_DEC_TRAIN = {true, true, true, true}, CONV_DEC_DECODE = {true, true, true, false}, CONV_DEC_TAIL = {false, true, false, false};
void conv_decoder_carve(Bump& ws, size_t R, int zd, ConvDecRuns runs, ConvDecWs& W);

// the decoder on R rows of z: fills W.d1 .. W.logit [R, 784]
int conv_decode_fwd(const ConvDecLayout& D, const ConvDecPacked& K, const float* params, const float* packed, const float* z, int R, ConvDecWs& W,
                    hipStream_t st);
// its two halves: up to W.u1 [R, 8, 8, 32] (decode.fc, deconv1 with its activation and zero pad: fills W.d1, d2, g0, c1, u1), and the last two stages
// from u1 as the four unfused launches (deconv2, logit_fn: fills W.c2, u2, c3, logit)
int conv_decode_head_fwd(const ConvDecLayout& D, const ConvDecPacked& K, const float* params, const float* packed, const float* z, int R, ConvDecWs& W,
                         hipStream_t st);
int conv_decode_tail_fwd(const ConvDecLayout& D, const ConvDecPacked& K, const float* params, const float* packed, const float* u1, int R, ConvDecWs& W,
                         hipStream_t st);
// the same two stages as ONE launch (conv_tail_kernel, csrc/convmodel.hip): u1 [R, 8, 8, 32] -> logit [R, 784]; b2 / b3: the biases of decode.deconv2 and
// decode.reparam.logit_fn in the parameter buffer, wt2 [CT_W2] / wt3 [CT_W3]: their weights (ConvTranspose2d layout [in, out, 5, 5]) as
// launch_conv_tail_pack re-lays them, on 16-byte boundaries of the packed buffer
constexpr size_t CT_W2 = 32 * 25 * 16, CT_W3 = 16 * 32;
int launch_conv_tail(const float* u1, const float* wt2, const float* b2, const float* wt3, const float* b3, int R, int act, float* logit, hipStream_t st);
int launch_conv_tail_pack(const float* w2, const float* w3, float* wt2, float* wt3, hipStream_t st);
// decoder backward from W.dlogit (and W.dzq = the part of dL/dz that does not pass through the decoder): fills dc3 / dp2 / dc2 / dp1 / dc1 / dg0 /
// dd2 / dd1 and W.dz
int conv_decoder_bwd(const ConvDecLayout& D, const ConvDecPacked& K, const float* packed, ConvDecWs& W, int R, hipStream_t st);
// the decoder's eight weight-gradient problems (z: the rows the forward decoded)
void conv_decoder_wgrads(const ConvDecLayout& D, const ConvDecWs& W, const float* z, int R, WgradList& wl);
}  // namespace ardae
