// Weight-normalised residual-conv models (ardae_model_desc.kind 5: ResConvIPVAE `--model resconvct-res`, 6: MNISTResConvAuxIPVAE
// `--model auxresconvct`, 12: MNISTResConvVAE `vae.py --model resconv`, 19: MNISTResConvAuxVAE `vae.py --model auxresconv`); csrc/model.hip dispatches
// to the families.  Noise: kind 5 [rows, noise_dim]; kind 6 [rows, noise_dim + z_dim] (rows [eps0 | eps], noise_dim = z0_dim); the hidden1a context of
// kind 6 is h [B, c_dim = h_dim] (ivae/auxresconv.py:125-132).
// The trunk, the decoder (models/vae/resconv.py:79-136), the residual block and the weight-norm backward are csrc/resmodel.hip's, declared here for the
// families that share them: kinds 5 / 6 (csrc/resmodel.hip), kind 12 (csrc/resvae.hip), kind 19 (csrc/auxresvae.hip).  A kind owns what stands between
// trunk and decoder - its Linears, their panels, their rows - in a layout, a packing and a workspace derived from the three structs below.
#pragma once
#include <utility>

#include "host_util.h"

namespace ardae {
extern const Family RES_FAMILY;

// Kind 12 (MNISTResConvVAE, `vae.py --model resconv`, models/vae/resconv.py): the same trunk and decoder with a plain Gaussian head.  The row is all
// it exports: the ardae_vae_* entry points (csrc/vaemodel.hip) reach its descriptor rules and bodies through the row's `gauss` member (csrc/vaemodel.h).
extern const Family RESVAE_FAMILY;
// Kind 19 (MNISTResConvAuxVAE, `vae.py --model auxresconv` / `auxresconvct`, models/vae/auxresconv.py): the Gaussian counterpart of kind 6 - kind 12's
// trunk and decoder with the two-stage posterior and the auxiliary decoder of csrc/auxvae.h's families.
extern const Family AUXRESVAE_FAMILY;

// ------------------------------------------------------------------------------------------------ layout
// plain: the operator is an nn.Linear (weight at `dir`, no scale, effective weight = weight): ResMLP(layer='linear')
struct WN { size_t dir, scale, bias; int O, I; bool norm; bool plain; };          // flat-parameter offsets; I = fan-in (C*9 for a conv)
struct Blk { WN a, h, s; bool conv; int Cin, Cout, stride, Hin, Hout; bool same; };   // a = *_0h, h = *_h1, s = *_01 (skip; absent when same: identity)

// the offset walk through the flat parameter buffer, in the reference's parameter order
struct ResWalk {
  size_t off = 0;
  WN wn(int O, int I, bool norm, bool plain = false) {
    WN w; w.O = O; w.I = I; w.norm = norm; w.plain = plain;
    w.dir = off; off += (size_t)O * I; w.scale = off; if (!plain) off += O; w.bias = off; off += O;
    return w;
  }
  Blk block(int Cout, int Cin, bool conv, int stride, int Hin, bool norm, bool plain = false, bool same = false) {
    Blk b; b.conv = conv; b.Cin = Cin; b.Cout = Cout; b.stride = stride; b.Hin = Hin; b.same = same;
    b.Hout = conv ? (Hin + 2 - 3) / stride + 1 : 1;
    const int I = conv ? Cin * 9 : Cin, Ih = conv ? Cout * 9 : Cout;
    b.a = wn(Cout, I, norm, plain); b.h = wn(Cout, Ih, norm, plain);
    if (same) { b.s = b.h; b.s.O = 0; } else b.s = wn(Cout, I, norm, plain);
    return b;
  }
  Lin lin(int out, int in) { return next_lin(off, out, in); }
};
// The shared part of a layout.  A kind's layout derives from it and walks in its constructor: trunk_blocks(w), its own members between trunk and
// decoder, decoder_blocks(w), (kind 19) its members behind the decoder, total = w.off.
struct ResLayout {
  int nd, zd, cdim, hdim;
  bool center;                   // do_center: the trunk sees 2x - 1 (desc.flags without ARDAE_MODEL_NO_CENTER)
  std::vector<Blk> trunk, dec;   // trunk: 5 conv + ResLinear(512 -> cdim); dec: 2 ResLinear + 5 conv
  size_t total = 0;
 protected:
  ResLayout(const ardae_model_desc& d, int cdim_) : nd(d.noise_dim), zd(d.z_dim), cdim(cdim_), hdim(d.h_dim), center(!(d.flags & ARDAE_MODEL_NO_CENTER)) {}
  void trunk_blocks(ResWalk& w) {
    trunk.push_back(w.block(16, 1, true, 2, 28, true));    // 28 -> 14
    trunk.push_back(w.block(16, 16, true, 1, 14, true));
    trunk.push_back(w.block(32, 16, true, 2, 14, true));   // 14 -> 7
    trunk.push_back(w.block(32, 32, true, 1, 7, true));
    trunk.push_back(w.block(32, 32, true, 2, 7, true));    // 7 -> 4
    trunk.push_back(w.block(cdim, 512, false, 1, 1, true));
  }
  void decoder_blocks(ResWalk& w) {
    dec.push_back(w.block(cdim, zd, false, 1, 1, true));
    dec.push_back(w.block(512, cdim, false, 1, 1, true));
    dec.push_back(w.block(32, 32, true, 1, 8, true));
    dec.push_back(w.block(32, 32, true, 1, 8, true));
    dec.push_back(w.block(16, 32, true, 1, 14, true));
    dec.push_back(w.block(16, 16, true, 1, 14, true));
    dec.push_back(w.block(1, 16, true, 1, 28, true));
  }
};

// offsets into the packed buffer
struct WNPk { size_t weff, inv, f, b; };
struct BlkPk { WNPk a, h, s; size_t bsum; size_t a_fi, a_fn, a_bi, s_fi, s_fn, s_bi; };   // *_fi / *_fn / *_bi: image half / noise half of a concat-input operator
struct LinPk { size_t f, b, fi, fn, bi, bn; };   // fi / fn: image / noise columns forward; bi / bn: their transposes
// the reservations of a packing, in pack order.  An operator's panels are packed from its effective weight: composed into the packed buffer at k.weff
// by res_pack's compose launch (weight norm), or the parameter itself (plain nn.Linear operator, whose weff / inv stay unused)
struct ResPackWalk {
  PackList& pl;
  size_t wn_panel(const WN& w, const WNPk& k, int col0, int nout, int kk, bool tr) {
    return pl.panel((w.plain ? w.dir : k.weff) + col0, w.I, nout, kk, tr, !w.plain);
  }
  WNPk wn(const WN& w) {
    WNPk k; k.weff = pl.take((size_t)w.O * w.I); k.inv = pl.take(w.O);
    k.f = wn_panel(w, k, 0, w.O, w.I, false); k.b = wn_panel(w, k, 0, w.I, w.O, true);
    return k;
  }
  BlkPk blk(const Blk& b, int split) {
    BlkPk k; k.a = wn(b.a); k.h = wn(b.h); k.s = b.same ? k.h : wn(b.s); k.bsum = pl.take(b.Cout);
    k.a_fi = k.a_fn = k.a_bi = k.s_fi = k.s_fn = k.s_bi = 0;
    if (split) {   // concat input [image part (split columns) | noise part]  (a concat block always has its projected skip: cdim + nd != Cout)
      const int nn = b.a.I - split;
      k.a_fi = wn_panel(b.a, k.a, 0, b.a.O, split, false); k.a_fn = wn_panel(b.a, k.a, split, b.a.O, nn, false); k.a_bi = wn_panel(b.a, k.a, 0, split, b.a.O, true);
      k.s_fi = wn_panel(b.s, k.s, 0, b.s.O, split, false); k.s_fn = wn_panel(b.s, k.s, split, b.s.O, nn, false); k.s_bi = wn_panel(b.s, k.s, 0, split, b.s.O, true);
    }
    return k;
  }
  LinPk lin(const Lin& l, int split) {
    LinPk k; pl.pair(l, k.f, k.b); k.fi = k.fn = k.bi = k.bn = 0;
    if (split) {
      k.fi = pl.panel(l.w, l.in, l.out, split, false); k.fn = pl.panel(l.w + split, l.in, l.out, l.in - split, false);
      k.bi = pl.panel(l.w, l.in, split, l.out, true); k.bn = pl.panel(l.w + split, l.in, l.in - split, l.out, true);
    }
    return k;
  }
};
// The shared part of a packing, cut as the layout: trunk_panels(P, w), the kind's own, decoder_panels(P, w), (kind 19) what follows.
struct ResPacked {
  std::vector<BlkPk> trunk, dec;
 protected:
  ResPacked() {}
  void trunk_panels(const ResLayout& P, ResPackWalk& w) { for (auto& b : P.trunk) trunk.push_back(w.blk(b, 0)); }
  void decoder_panels(const ResLayout& P, ResPackWalk& w) { for (auto& b : P.dec) dec.push_back(w.blk(b, 0)); }
};
// floats of resconv_mid_kernel's weights in a packed buffer (kind 19 reserves them; launch_mid_pack fills them)
constexpr int RM_WTOTAL = (2 * 288 + 4 * 144) * 16;

// the rules kinds 12 and 19 share (input_dim 784, h_dim = c_dim >= 1, z_dim >= 1, n_layers 1, ELU, flags within ARDAE_MODEL_NO_CENTER); the messages
// name d->kind, the class and where the reference asserts ELU.  Each kind adds its noise_dim rule in front.
int res_gauss_desc_check(const ardae_model_desc* d, const char* cls, const char* elu_assert);

// ------------------------------------------------------------------------------------------------ workspace
// saved activations of one block
struct BlkBuf { float *colsx, *hmid, *colsh, *out; };
// scratch of one block's backward (reused from block to block) and the gradient destinations of its three operators
struct BwdScratch { float *g, *dh, *dcols; };
struct WnGrad { float* dW; float* db; float beta; };   // beta: accumulate into the destination (plain operators write the gradient buffer itself)
struct BlkGrad { WnGrad a, h, s; };
// The buffers every kind has.  A kind's rows (its heads, draws, seeds, z) are a struct derived from this one in the kind's file.
struct ResWs {
  // trunk (B images)
  float* x2; std::vector<BlkBuf> tb; float *flat, *inp;             // 2x-1, block buffers, NCHW-flattened conv output [B,512], trunk output [B,cdim]
  // decoder (R images)
  std::vector<BlkBuf> db; float *d4, *u8, *c7, *u14, *u28;          // block buffers; NHWC 4x4x32, upsampled / cropped maps
  float *rec_row, *pri_row, *dlogit, *dzq;
  // backward scratch
  BwdScratch sc; float *da, *dbuf, *dflat, *dinp, *dR0, *dR1, *dB0, *dB1, *dB2;
  float* dweff; float* dbias; float* wscratch; size_t wscratch_floats;
};
// which of the decoder's blocks run as their own launches - dec[0 .. 3] always, mid: dec[4] and dec[5] (else resconv_mid_kernel stands for them and
// for c7, u14), tail: dec[6] (else resconv_tail_kernel stands for it and u28) - and whether every block keeps its own columns (a backward reads them)
// or all share ONE columns scratch, the widest running block's
struct DecRuns { bool mid, tail, keep; };

size_t blk_rows(const Blk& b, int images);
void blk_carve(const Blk& b, int images, Bump& ws, BlkBuf& u);
// the pieces of a kind's carve, in this order with the kind's own takes in between: the trunk's forward buffers on B images; the decoder's on R rows
// (dec[5]'s output exists whatever runs); the loss rows and the backward's scratch, the weight-gradient scratch sized for the widest block and for
// head_wgrad_floats, what the kind's own weight-gradient list needs.  (A kind's carve(P, K, ws, ..., W) leaves the packing unread: Entry<> and
// ip_workspace_floats call every family's carve that way.)
void res_trunk_carve(const ResLayout& P, Bump& ws, int B, ResWs& W);
void res_decoder_carve(const ResLayout& P, Bump& ws, size_t R, DecRuns runs, ResWs& W);
void res_bwd_carve(const ResLayout& P, Bump& ws, int B, size_t R, size_t head_wgrad_floats, ResWs& W);
size_t wgrad_scratch_floats(int M, int O, int I);

// ------------------------------------------------------------------------------------------------ forward, backward, pack
// forward of a residual block on `images` images (conv) / rows (linear); x: [images*Hin*Hin, Cin]; act_out: ELU after the block or none
int blk_fwd(const Blk& b, const BlkPk& k, const float* params, const float* packed, const float* x, int images, int act_out, BlkBuf& u, hipStream_t st);
// backward of a block: d_out [R, Cout] (gradient w.r.t. the block's output AFTER act_out) -> d_x [rows_in, Cin] (may be null)
int blk_bwd(const Blk& b, const BlkPk& k, const float* packed, const float* x, int images, int act_out, const BlkBuf& u, const float* d_out, float* d_x,
            const BwdScratch& sc, const BlkGrad& gr, float* wscratch, size_t wscratch_floats, hipStream_t st);
// assign splits + scratch (the scratch is reused from batch to batch; the batch size is the wgrad_splits hint) and launch,
// at most ARDAE_WGRAD_MAX_PROBLEMS per batch
int flush_wgrad(WgradList& wl, float* scratch, size_t scratch_floats, hipStream_t st);

// x [B, 784] -> W.inp [B, cdim]
int res_trunk_fwd(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* x, int B, ResWs& W, hipStream_t st);
// upsample x2 + dec[6] on R images in one launch: y14 [R, 14, 14, 16] (dec[5]'s output after its ELU) -> logits [R, 784]
int tail_fused(const Blk& b, const BlkPk& k, const float* params, const float* packed, const float* y14, int R, float* logits, hipStream_t st);
// crop + upsample + dec[4] + dec[5] on R images in one launch: y8 [R, 8, 8, 32] (dec[3]'s output after its ELU) -> y14 [R, 14, 14, 16];
// mid_w: the RM_WTOTAL floats launch_mid_pack has written
int mid_fused(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* mid_w, const float* y8, int R, float* y14,
              hipStream_t st);
// the 14 x 14 stage as its launches: y8 [R, 8, 8, 32] -> u5.out [R, 14, 14, 16]
int mid_unfused(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* y8, int R, float* c7, float* u14, BlkBuf& u4,
                BlkBuf& u5, hipStream_t st);
// which tail / 14 x 14 stage the decode-only path of kinds 12 / 19 runs (variant 0 of ardae_resconv_tail / _mid; the mode-2 workspace is sized for the
// answer): the fused kernel, unless ARDAE_RESCONV_TAIL_UNFUSED=1 / ARDAE_RESCONV_MID_UNFUSED=1 under ARDAE_DEBUG_KNOBS=1
bool tail_fused_default();
bool mid_fused_default();
// decoder on R rows: z [R, zd] -> logits [R, 784] (null: they stay in W.db[6].out)
// fused_tail (kind 12's decode-only path): the last upsampling and dec[6] as resconv_tail_kernel, which writes `logits` itself
// fused_mid_w (kind 19's decode-only path; null: unfused): the crop, the 7 -> 14 upsampling, dec[4] and dec[5] as resconv_mid_kernel on these weights
int res_decoder_fwd(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* z, int R, ResWs& W, float* logits,
                    hipStream_t st, bool fused_tail = false, const float* fused_mid_w = nullptr);

// one operator of wn_backward_kernel's launch
struct WnBwdItem {
  const float* dW; const float* dir; const float* scale; const float* inv; const float* db;   // db: [O] bias gradient (scratch)
  float* gdir; float* gscale; float* gbias;
  int O, I, norm;
};
// gradient destinations of a WN operator inside the dweff / dbias scratch
struct GradMap {
  float* dweff; float* dbias; size_t boff = 0;
  std::vector<WnBwdItem> items;
  const float* params; const float* packed; float* grads;
  float grads_beta = 0.f;
  WnGrad wn(const WN& w, const WNPk& k);
  BlkGrad blk(const Blk& b, const BlkPk& k) { BlkGrad g; g.a = wn(b.a, k.a); g.h = wn(b.h, k.h); g.s = b.same ? g.h : wn(b.s, k.s); return g; }
};
GradMap grad_map(ResWs& W, const float* params, const float* packed, float* grads, float grads_beta);
// the decoder's backward on R rows from W.dlogit (z: the rows it decoded): every block's weight gradients into gm's scratch, dz (added to what the
// loss kernel left) in W.dzq
int res_decoder_bwd(const ResLayout& P, const ResPacked& K, const float* packed, const float* z, ResWs& W, int R, GradMap& gm, hipStream_t st);
// the trunk's backward on B images from W.dinp (the gradient at its output, after the ELU), then dL/dW -> dL/d(direction, scale) and the bias
// gradients of every weight-normalised operator gm has handed out
int res_trunk_wn_bwd(const ResLayout& P, const ResPacked& K, const float* packed, ResWs& W, int B, GradMap& gm, float grads_beta, hipStream_t st);

// ardae_model_pack: the effective weights and bias sums of the trunk's, `head`'s (kind 5) and the decoder's blocks, composed into the packed buffer,
// then pl's pack launch, which reads them
using HeadBlks = std::vector<std::pair<const Blk*, const BlkPk*>>;
int res_pack(const ResLayout& P, const ResPacked& K, const HeadBlks& head, PackList& pl, hipStream_t st);
// resconv_mid_kernel's B operands at mid_w, from the effective weights res_pack's compose launch has written (kind 19's pack runs it behind res_pack)
int launch_mid_pack(const ResPacked& K, float* packed, size_t mid_w, hipStream_t st);
// Family::pack of a kind whose own operators are plain Linears
template <class Layout, class Packed> int res_family_pack(const ardae_model_desc& d, const float* params, float* packed, hipStream_t st) {
  const Layout P(d);
  PackList pl(params, packed);
  const Packed K(P, pl);
  return res_pack(P, K, {}, pl, st);
}

// What ardae_resconv_tail / ardae_resconv_mid (csrc/resmodel.hip) read of kinds 12 / 19: the shared parts of the kind's layout and packing
struct ResDecoderView { ResLayout P; ResPacked K; size_t mid_w; };      // mid_w: kind 19
ResDecoderView resvae_decoder_view(const ardae_model_desc& d);          // csrc/resvae.hip
ResDecoderView auxresvae_decoder_view(const ardae_model_desc& d);       // csrc/auxresvae.hip
}  // namespace ardae
