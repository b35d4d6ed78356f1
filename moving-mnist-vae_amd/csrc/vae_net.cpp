#include "vae_net.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "conv_ops.hpp"

namespace mmvae {

#define MM_TRY(expr)            \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ < 0) return rc__;  \
  } while (0)

static inline long align_up(long v, long a) { return (v + a - 1) / a * a; }
static inline int down_size(int H, int k, int s, int p) { return conv_down_size(H, k, s, p); }

// ------------------------------------------------------------------------------------------------ construction
void Net::add_entry(const std::string& name, std::initializer_list<int> shape, int kind, long off) {
  Entry e; e.name = name; e.ndim = (int)shape.size(); e.kind = kind; e.offset = off;
  int i = 0; for (int d : shape) e.shape[i++] = d;
  for (; i < 4; ++i) e.shape[i] = 1;
  entries.push_back(e);
}

ConvW Net::add_conv(const std::string& name, int D0, int D1, int k, int s, int p, bool pack, bool transposed) {
  ConvW w; w.off = n_params; w.D0 = D0; w.D1 = D1; w.k = k; w.s = s; w.p = p; w.packD = w.packU = -1; w.tr = transposed;
  add_entry(name, {D0, D1, k, k}, EK_PARAM, n_params);
  const long numel = (long)D0 * D1 * k * k;
  n_params += numel;
  if (numel > max_w) max_w = numel;
  if (pack) { w.packD = n_packed; n_packed += align_up(numel, 8); w.packU = n_packed; n_packed += align_up(numel, 8); }
  if (cfg.fp8 && pack && D0 >= 64 && D1 >= 64 && D0 % 64 == 0 && D1 % 64 == 0) {
    // candidate; settle_layout() confirms it once the layer's place in the net (Hl) is known
    // static scale: PyTorch's default init is U(+-1/sqrt(D1*k*k)) for both weight layouts; bring that bound to ~16..32 (e4m3 normal range)
    w.fp8 = true;
    int e = 0; while ((float)(1 << e) < 16.f * std::sqrt((float)D1 * k * k)) ++e;
    w.wscale = (float)(1 << e);
  }
  return w;
}

// An fp8 layer's forward weights are e4m3 bytes that only the fp8 form of deep2_conv_kernel reads: keep the flag only where that kernel
// takes the layer's FORWARD launch (e.g. z = 192 makes decoder.conv1 a 3-chunk row, which it does not) -- the others stay bf16 layers.
// So do the layers on 2x2 / 4x4 maps whose forward the bf16 position-major kernel takes: it is faster there than the e4m3 deep2 form (with them
// in fp8 the mode ran at 0.96x of bf16 in round 4) -- fp8 arithmetic stays where it pays.
//
// The layouts of the two packs follow: fragment-major where deep2_conv_kernel takes the launch of that form at the layer's place in the net
// (the e4m3 form for the forward direction of an fp8 layer).  The up form of a 1x1 stride-2 shortcut has stride phases without a tap: in this
// net it only ever accumulates into (or rides along with) the main path's data gradient, so those phases are skipped.
void Net::settle_layout(ConvW& w) const {
  if (w.Hl <= 0) { if (w.fp8) { w.fp8 = false; w.wscale = 1.f; } return; }
  const ConvGeom g{w.D0, w.D1, w.k, w.s, w.p};
  const ConvLayout dn = op_down_layout(dt(), g, w.Hl, w.Hl), up = op_up_layout(dt(), g, w.Hl, w.Hl, 1);
  const ConvLayout& fwd = w.tr ? up : dn;
  if (w.fp8 && (fwd.pos || !fwd.fp8)) { w.fp8 = false; w.wscale = 1.f; }
  w.fragD = (w.fp8 && !w.tr) ? dn.fp8 : dn.frag;
  w.fragU = (w.fp8 && w.tr) ? up.fp8 : up.frag;
}

Bn Net::add_bn(const std::string& prefix, int C) {
  Bn b; b.C = C;
  b.g_off = n_params; add_entry(prefix + ".weight", {C}, EK_PARAM, n_params); n_params += C;
  b.b_off = n_params; add_entry(prefix + ".bias", {C}, EK_PARAM, n_params); n_params += C;
  b.rm_off = n_bnbuf; add_entry(prefix + ".running_mean", {C}, EK_BN_F32, n_bnbuf); n_bnbuf += C;
  b.rv_off = n_bnbuf; add_entry(prefix + ".running_var", {C}, EK_BN_F32, n_bnbuf); n_bnbuf += C;
  b.nbt_idx = n_nbt; { Entry e; e.name = prefix + ".num_batches_tracked"; e.ndim = 0; e.kind = EK_BN_I64; e.offset = n_nbt;
                       for (int i = 0; i < 4; ++i) e.shape[i] = 1; entries.push_back(e); } n_nbt += 1;
  b.ws = n_bnws; n_bnws += b.scratch_floats();
  return b;
}

Net::Net(const NetCfg& c) : cfg(c) {
  const int S = c.S;
  // ---- encoder (model.py:89-112)
  H1 = W1 = down_size(S, 5, 2, 2);
  stem = add_conv("encoder.conv1.weight", 32, c.in_ch, 5, 2, 2, false);
  bn0 = add_bn("encoder.bn1", 32);
  int inpl = 32, H = H1;
  const int planes[4] = {32, 64, 128, 256};
  const int nb = c.blocks < 1 ? 1 : c.blocks;
  for (int i = 0; i < 4; ++i) {
    for (int b = 0; b < nb; ++b) {
      // _make_layer (model.py:132-146): block 0 strides and carries the 1x1 downsample shortcut, the others keep the shape
      Block B;
      const std::string p = "encoder.layer" + std::to_string(i + 1) + "." + std::to_string(b) + ".";
      const int st = b == 0 ? 2 : 1;
      B.identity = b > 0;
      B.Cin = inpl; B.C = planes[i]; B.Hin = B.Win = H; B.Hout = B.Wout = down_size(H, 3, st, 1); B.Hmid = B.Wmid = B.Hout;
      B.c1 = add_conv(p + "conv1.weight", planes[i], inpl, 3, st, 1, true);       // conv3x3 (:29,:98-101)
      B.b1 = add_bn(p + "bn1", planes[i]);
      B.c2 = add_conv(p + "conv2.weight", planes[i], planes[i], 3, 1, 1, true);  // conv3x3 (:33)
      B.b2 = add_bn(p + "bn2", planes[i]);
      if (!B.identity) {
        B.cs = add_conv(p + "downsample.0.weight", planes[i], inpl, 1, 2, 0, true);  // conv1x1 stride 2 (:135-138)
        B.bs = add_bn(p + "downsample.1", planes[i]);
      }
      B.c1.Hl = B.Hin; B.c2.Hl = B.Hout; B.cs.Hl = B.Hin;
      inpl = planes[i]; H = B.Hout;
      enc.push_back(B);
    }
  }
  Hf = Wf = H;
  head_mu = add_conv("encoder.conv_mu.weight", c.z, 256, 1, 1, 0, false);
  if (c.need_logvar) head_lv = add_conv("encoder.conv_logvar.weight", c.z, 256, 1, 1, 0, false);
  const long hp = align_up((long)c.z * Hf * Wf * 256, 8);
  head_pack_mu = n_packed; n_packed += hp;
  head_pack_lv = n_packed; n_packed += hp;
  head_pack_dg = n_packed; n_packed += align_up(2L * c.z * 256, 8);
  stem_pack = n_packed; n_packed += 32L * 25 * 8;
  l1c2_flip = n_packed; n_packed += 32L * 9 * 32;          // encoder.layer1.conv2 as [cin][flipped tap][cout]: its data gradient as a forward conv
  tail_pack_f = n_packed; n_packed += 16L * 9 * 16;
  tail_pack_d = n_packed; n_packed += 16L * 9 * 8;
  // ---- decoder (model.py:154-179)
  dec_param_off = n_params;
  dstem = add_conv("decoder.conv1.weight", c.z, 128, 2, 2, 0, true, true);   // k2 s1 p0 on a 1x1 input == k2 s2 p0
  dstem.Hl = 2;
  dbn0 = add_bn("decoder.bn1", 128);
  nup = S > 32 ? 5 : 4;                                               // :169
  const int ups[5] = {128, 64, 32, 16, 16};
  int cin = 128; H = 2;
  for (int i = 0; i < nup; ++i) {
    for (int b = 0; b < nb; ++b) {
      // _make_up_block (model.py:196-209): the extra blocks come FIRST and the upsampling block last.  The reference builds the extra
      // ones as block(in, out) with the 2x ConvTranspose2d main path and an identity shortcut, which cannot run (shape mismatch,
      // :205-206); here they keep the stage's input shape: conv1x1 -> BN -> ReLU -> conv3x3 -> BN, + identity, ReLU.
      Block B;
      const std::string p = "decoder.uplayer" + std::to_string(i + 1) + "." + std::to_string(b) + ".";
      B.identity = b < nb - 1;
      if (B.identity) {
        B.Cin = cin; B.C = cin; B.Hin = B.Win = H; B.Hmid = B.Wmid = H; B.Hout = B.Wout = H;
        B.c1 = add_conv(p + "conv1.weight", cin, cin, 1, 1, 0, true);
        B.b1 = add_bn(p + "bn1", cin);
        B.c2 = add_conv(p + "conv2.weight", cin, cin, 3, 1, 1, true);           // Conv2d (out,in,3,3): the shape-preserving main path
        B.b2 = add_bn(p + "bn2", cin);
        B.c1.Hl = H; B.c2.Hl = H;
      } else {
        B.Cin = cin; B.C = ups[i]; B.Hin = B.Win = H; B.Hmid = B.Wmid = H; B.Hout = B.Wout = 2 * H;
        B.c1 = add_conv(p + "conv1.weight", ups[i], cin, 1, 1, 0, true);        // 1x1 (:60)
        B.b1 = add_bn(p + "bn1", ups[i]);
        B.c2 = add_conv(p + "conv2.weight", ups[i], ups[i], 4, 2, 1, true, true);      // ConvT k4 s2 p1 (:62-65)
        B.b2 = add_bn(p + "bn2", ups[i]);
        B.cs = add_conv(p + "upsample.0.weight", cin, ups[i], 4, 2, 1, true, true);    // ConvT k4 s2 p1 (:198-201)
        B.bs = add_bn(p + "upsample.1", ups[i]);
        B.c1.Hl = H; B.c2.Hl = 2 * H; B.cs.Hl = 2 * H;
        cin = ups[i]; H = 2 * H;
      }
      dec.push_back(B);
    }
  }
  Sd = H;
  // fp8 mode: the two largest activations of the step (the last up-block's branch outputs at 64x64: 671 MB each in bf16 at 5120 frames, written
  // once and read three times) are STORED as e4m3 bytes where the four stream kernels that touch them run (convT4_stream -> tail_fwd_stream,
  // tail_reduce_mfma, join_bwd_stream).  A static weight scale of 16 puts their values mid-range; the BatchNorms behind absorb it exactly
  // (the same mechanism as an fp8 layer's weight scale).
  if (cfg.fp8 && !dec.empty()) {
    Block& L = dec.back();
    if (!L.identity && L.C == 16 && L.Cin == 16 && L.Hin == 32 && Sd == 64 && c.out_ch == 1 && convT4_stream_ok(DT_BF16, 16, 16, 4, 2, 1, 32, 32) &&
        tail_fwd_stream_ok(DT_BF16, 1, 64, 64) && join_bwd_stream_ok(DT_BF16, 1, 16, 32, 64)) {
      store8 = true;
      L.c2.wscale = 16.f; L.cs.wscale = 16.f;
    }
  }
  settle_layout(dstem);
  for (Block& B : enc) { settle_layout(B.c1); settle_layout(B.c2); if (!B.identity) settle_layout(B.cs); }
  for (Block& B : dec) { settle_layout(B.c1); settle_layout(B.c2); if (!B.identity) settle_layout(B.cs); }
  tail = add_conv("decoder.conv2.weight", c.out_ch, 16, 3, 1, 1, false);
  tail_bias = n_params; add_entry("decoder.conv2.bias", {c.out_ch}, EK_PARAM, n_params); n_params += c.out_ch;
  bn_out = add_bn("decoder.bn2", c.out_ch);
}

Net::~Net() {
  if (side_state_ != 1) return;
  // work still queued on the side streams belongs to buffers the caller may free next: drain first
  if (side_) { (void)hipStreamSynchronize(side_); (void)hipStreamDestroy(side_); }
  for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : blk_ev_) if (e) (void)hipEventDestroy(e);
  if (gram_ev_) (void)hipEventDestroy(gram_ev_);
  (void)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ planning
size_t Net::workspace_bytes(int N) { return plan(N).bytes; }

const Plan& Net::plan(int N) {
  if (plan_.N == N) return plan_;
  Plan P; P.N = N;
  long cur = 0, maxact = 0;
  const long e = (long)esz();
  auto take = [&](long bytes) { long o = cur; cur = align_up(cur + std::max(bytes, 16L), 256); return o; };
  auto act = [&](long elems) { maxact = std::max(maxact, elems * e); return take(elems * e); };
  P.x_t = act((long)N * cfg.in_ch * cfg.S * cfg.S);
  P.y0 = act((long)N * H1 * W1 * 32);
  for (Block& B : enc) {
    const long n = (long)N * B.Hout * B.Wout * B.C;
    B.y1 = act(n); B.y2 = act(n); B.ys = B.identity ? 0 : act(n); B.out = act(n);
  }
  P.enc_t = act((long)N * cfg.z);
  P.y0d = act((long)N * 4 * 128);
  P.act0d = cfg.blocks > 1 ? act((long)N * 4 * 128) : 0;
  for (Block& B : dec) {
    const long n = (long)N * B.Hout * B.Wout * B.C;
    B.y1 = act((long)N * B.Hin * B.Win * B.C); B.y2 = act(n); B.ys = B.identity ? 0 : act(n); B.out = act(n);
  }
  P.cvec = take(512 * 4);
  P.r_raw = take((long)N * cfg.out_ch * Sd * Sd * 4);
  P.d_raw = take((long)N * cfg.out_ch * Sd * Sd * 4);
  // im2col of the 1-channel image; in_channels > 1: the image as NHWC with 16 zero-padded channels (the generic weight gradient's G operand)
  P.col = act(cfg.in_ch == 1 ? (long)N * H1 * W1 * 32 : (long)N * cfg.S * cfg.S * 16);
  P.packed = take(n_packed * e);
  P.bnws = take(n_bnws * 4);
  P.partials = take(2 * kPartialFloats * 4);       // second half: the shortcut branch running on the side stream
  P.syncbuf = take(2 * 1024 * 4);
  for (int i = 0; i < 2; ++i) P.g[i] = take(maxact);
  for (int i = 0; i < 2; ++i) { P.dy1[i] = take(maxact); P.dy2[i] = take(maxact); P.dys[i] = take(maxact); }
  for (int i = 0; i < 2; ++i) {        // private dy sets of the two encoder blocks the backward pass visits first
    const Block& B = enc[enc.size() - 2 + i];
    const long nb = (long)N * B.Hout * B.Wout * B.C * e;
    P.edy1[i] = take(nb); P.edy2[i] = take(nb); P.edys[i] = take(nb);
  }
  P.da1 = take(maxact);
  P.dh = take((long)N * 2 * cfg.z * e);
  P.wscratch = take((long)kWgradScratchBytes);
  P.wscratch2 = take(2L * 1024 * 4096 * 4);           // partial images of the fused passes on the caller's stream: 512 blocks x ([16][32][16] + [16][32]) f32 (wgrad_stream), 2 x 1024 x [16][16][16] (join_bwd_stream)
  P.stem_R = take(1024 * 8);
  P.stem_gram = take(1024L * stem_bwd_part_floats() * 4);
  P.bytes = (size_t)cur;
  settle_routes(N, P.route);
  plan_ = P;
  return plan_;
}

static inline ConvGeom geom(const ConvW& w) { return ConvGeom{w.D0, w.D1, w.k, w.s, w.p}; }
// Which kernel takes each launch of a train step at batch size N: the only place that asks the kernels' shape predicates (the constructor's store8
// guess aside).  One field per decision; the rules at the end are what forward and backward must agree on about what the forward stored.
void Net::settle_routes(int N, NetRoute& R) {
  const int nd = (int)dec.size();
  R = NetRoute(); R.store8 = store8;
  R.stem_fwd_stream = cfg.in_ch == 1 && stem_fwd_stream_ok(dt(), cfg.S);
  // the stem's backward in one pass (stem_bwd.hip); where the shape does not fit: reduce -> apply -> im2col -> wgrad
  // (measured: im2col + 1x1 weight gradient 0.39 ms, a planar-G patch-tile path 0.42 ms)
  R.stem_bwd_fused = cfg.in_ch == 1 && stem_bwd_fusable(cfg.S);
  for (size_t i = 0; i < enc.size(); ++i) {
    Block& B = enc[i];
    BlockRoute& r = B.r = BlockRoute();
    const ConvW &g = B.c1, &gs = B.cs;
    const bool plain = !B.identity && !g.fp8 && !gs.fp8;
    // encoder.layer1 (32 -> 32 channels, bf16): conv1 AND the 1x1 shortcut from ONE read of the block input, conv2 likewise a per-wave
    // stream (conv_fstream.hip); both BatchNorms finalise on the caller's stream
    r.fwd_c1_cs_stream = plain && gs.k == 1 && gs.s == 2 && conv3_stream_ok(dt(), B.Cin, B.C, g.k, g.s, g.p, B.Hin, B.Win);
    r.fwd_c2_stream = !B.c2.fp8 && conv3_stream_ok(dt(), B.C, B.C, B.c2.k, B.c2.s, B.c2.p, B.Hout, B.Wout);
    // conv1 (3x3 s2) + 1x1 s2 shortcut weight gradients in one stream pass: encoder.layer1's shape (bf16, 32 -> 32 channels, 32x32 -> 16x16)
    r.bwd_pair_wgrad = plain && dt() == DT_BF16 && g.k == 3 && g.s == 2 && g.p == 1 && gs.k == 1 && gs.s == 2 && gs.p == 0 && g.D0 == 32 &&
                       g.D1 == 32 && gs.D0 == 32 && gs.D1 == 32 && B.Hout == 16 && B.Hin == 32;
    // encoder.layer1 (the block the step ends on): conv2's weight gradient is a stream pass, whose reduce can wait (encoder_bwd says for what)
    r.bwd_c2_late_reduce = i == 0 && !B.c2.fp8 && op_wgrad_is_stream(dt(), geom(B.c2), MapIn::shape(B.Hout, B.Wout), MapIn::shape(B.Hout, B.Wout, true), N);
    // encoder.layer1.conv2's data gradient + bn1's backward sums in one stream pass (bf16, 32 -> 32 channels, 16x16 maps, one block per stage)
    r.bwd_c2_dgrad_stream = i == 0 && !B.identity && r.fwd_c2_stream;
  }
  // The stem's backward recomputes its incoming gradient (encoder.layer1's conv1 3x3 s2 + 1x1 s2 shortcut data gradients) instead of reading it:
  // bf16, 64x64 images, the reference's first stage (32 -> 32 channels, strided block with a 1x1 shortcut), row-major packed weights
  const Block& E = enc[0];
  R.stem_dg_fused = R.stem_bwd_fused && stem_bwd_dg_ok(dt(), cfg.S) && E.r.bwd_pair_wgrad && E.c1.wscale == 1.f && E.cs.wscale == 1.f && !E.c1.fragU &&
                    !E.cs.fragU && H1 == 32;
  // The tail conv's input gradient is not materialised where the shape allows: the last up-block's join backward recomputes it from d_raw
  // (launch_tail_join_bwd_*) -- as one pass over the whole block (conv_joinbwd.hip: dy2 / dys are produced row by row inside the kernel that consumes
  // them -- both ConvTranspose2d weight gradients, both data gradients, bn1's backward sums -- and never stored) or as reduce -> apply
  Block& L = dec.back();
  R.tail_bwd_fused = L.C == 16 && tail_join_fusable(dt(), cfg.out_ch, N, Sd, Sd);
  const bool last_js = R.tail_bwd_fused && !L.identity && !L.c2.fp8 && !L.cs.fp8 && !L.c1.fp8 && L.Cin == 16 && join_bwd_stream_ok(dt(), cfg.out_ch, L.C, L.Hin, L.Hout);
  for (int i = 0; i < nd; ++i) {
    Block& B = dec[i];
    BlockRoute& r = B.r = BlockRoute();
    r.bwd_join_stream = last_js && i == nd - 1;
    // the two ConvTranspose2d forwards as per-wave streams (conv_fstream.hip)
    r.fwd_cs_stream = !B.identity && !B.cs.fp8 && convT4_stream_ok(dt(), B.cs.D0, B.cs.D1, B.cs.k, B.cs.s, B.cs.p, B.Hin, B.Win);
    r.fwd_c2_stream = !B.identity && !B.c2.fp8 && convT4_stream_ok(dt(), B.c2.D0, B.c2.D1, B.c2.k, B.c2.s, B.c2.p, B.Hin, B.Win);
    // the join, fused with the next block's 1x1 conv1 and bn1's statistics where that block's conv1 is 16-wide (uplayer3 -> 4, uplayer4 -> 5):
    // the joined row is the conv's operand while it is in LDS -- one launch and one pass over `out` fewer than join -> conv
    if (i + 1 < nd && !B.identity && !dec[i + 1].identity) {
      const ConvW& n1 = dec[i + 1].c1;
      r.fwd_join_conv1 = !n1.fp8 && n1.k == 1 && n1.s == 1 && n1.D1 == B.C && !n1.fragD && n1.wscale == 1.f &&
                         join_conv1_fwd_ok(dt(), B.C, n1.D0, (long)N * B.Hout * B.Wout);
    }
    // Where the shape allows (uplayer4 / uplayer5: 16 output channels, 16x16 -> 32x32 or 32x32 -> 64x64, bf16) dgrad and wgrad of a ConvT
    // are ONE pass over its dy tensor on the caller's stream (wgrad_stream_kernel with DG): dy2 / dys (671 MB each at N = 5120 in
    // uplayer5) are read once instead of twice.  (Not asked where join_bwd_stream takes the whole block.)
    const bool own = !B.identity && !r.bwd_join_stream;
    const MapIn small = MapIn::shape(B.Hin, B.Win), small_pro = MapIn::shape(B.Hin, B.Win, true), large = MapIn::shape(B.Hout, B.Wout);
    r.bwd_fuse_c2 = own && !B.c2.fp8 && op_bwd_fusable(dt(), geom(B.c2), small, large, N);
    r.bwd_fuse_cs = own && !B.cs.fp8 && op_bwd_fusable(dt(), geom(B.cs), small, large, N) && B.C == 16;
    // Join-gradient form of a block's backward (blocks on 16-wide maps, uplayer4): the block above hands down its input gradient already masked
    // by this block's join ReLU (conv1_bwd_stream_kernel, MASK: join_bwd_stream's block), the BatchNorm-backward reduce runs unmasked, and dy2 / dys
    // are evaluated by the loaders of the two fused passes -- the bn_bwd_apply launch (840 MB at N = 5120) and both dy tensors disappear.
    r.bwd_join_grad = last_js && i == nd - 2 && dt() == DT_BF16 && join_grad_ && own && B.C == 16 && !B.c2.fp8 && !B.cs.fp8 && !B.c1.fp8 &&
                      !(i == 0 && cfg.blocks <= 1) && op_bwd_fusable_jg(dt(), geom(B.c2), small_pro, large, N, false, true) &&
                      op_bwd_fusable_jg(dt(), geom(B.cs), small, large, N, true, false);
  }
  // Last up-block forward as one kernel (join + tail conv, the joined activation is never stored); the backward then needs the recomputing wgrad
  // (tail_wg_in_reduce: inside the join-backward reduce pass) and the recomputing join backward.  Shapes it does not take keep join -> conv.
  // (N does not enter the geometry checks beyond the tile count limit, which the plan's maximum batch already satisfies)
  const bool fused = L.C == 16 && tail_fwd_fusable(dt(), cfg.out_ch, 1, Sd, Sd) && tail_join_fusable(dt(), cfg.out_ch, 1, Sd, Sd);
  const bool stream = tail_fwd_stream_ok(dt(), cfg.out_ch, Sd, Sd);
  // The up5_tail_fwd route: that kernel recomputes both ConvTranspose2d outputs anyway and STORES them (y2 / ys, for the backward pass) beside its
  // LDS-bound work, so the two ConvTranspose2d launches in front of it only take the batch statistics (fwd_stats_only: y == nullptr, no 1.34 GB of
  // stores in front of the join).  In eval mode the BatchNorms are folded and nothing reads y2 / ys: no launches, no stores.
  L.r.fwd_stats_only = fused && !R.store8 && stream && up5_tail_fwd_ok(dt(), cfg.out_ch, L.C, L.Cin, L.Hin, L.Hout) && L.r.fwd_c2_stream && L.r.fwd_cs_stream;
  R.tail_fwd = !fused ? TAIL_GATHER : L.r.fwd_stats_only ? TAIL_UP5 : stream ? TAIL_STREAM : TAIL_JOIN;
  R.tail_wg_in_reduce = fused && R.tail_bwd_fused;
  // ---- what the forward stored is what the backward reads (the first broken rule is reported)
  if (R.store8 && R.tail_fwd == TAIL_GATHER) R.refused = "fp8 storage of the last up-block needs the fused tail kernels";
  else if (R.store8 && R.tail_fwd != TAIL_STREAM) R.refused = "fp8 storage of the last up-block needs tail_fwd_stream";
  else if (R.store8 && !R.tail_wg_in_reduce) R.refused = "fp8 storage of the last up-block needs the fused tail backward";
  else if (R.tail_fwd != TAIL_GATHER && !R.tail_wg_in_reduce) R.refused = "decoder_bwd: the fused tail forward (no stored join) needs the fused tail backward";
  else if (R.store8 && !last_js) R.refused = "fp8 storage of the last up-block needs join_bwd_stream";
  for (const Block& B : dec)
    if (!R.refused && B.r.bwd_join_grad && !(B.r.bwd_fuse_c2 && B.r.bwd_fuse_cs)) R.refused = "decoder_bwd: the join-gradient form needs both fused passes";
}

int Net::describe_routes(int N, std::string& out) {
  const NetRoute& R = plan(N).route;
  if (R.refused) { set_error("%s", R.refused); return MMVAE_ERR_UNSUPPORTED; }
  const int nb = cfg.blocks < 1 ? 1 : cfg.blocks;
  auto line = [&](const std::string& name, std::initializer_list<std::pair<const char*, int>> fields) {
    out += name + ":";
    for (const auto& f : fields) out += std::string(" ") + f.first + "=" + std::to_string(f.second);
    out += "\n";
  };
  out.clear();
  for (size_t i = 0; i < enc.size(); ++i) {
    const BlockRoute& r = enc[i].r;
    line("encoder.layer" + std::to_string(i / nb + 1) + "." + std::to_string(i % nb),
         {{"fwd_c1_cs_stream", r.fwd_c1_cs_stream}, {"fwd_c2_stream", r.fwd_c2_stream}, {"bwd_pair_wgrad", r.bwd_pair_wgrad},
          {"bwd_c2_late_reduce", r.bwd_c2_late_reduce}, {"bwd_c2_dgrad_stream", r.bwd_c2_dgrad_stream}});
  }
  for (size_t i = 0; i < dec.size(); ++i) {
    const BlockRoute& r = dec[i].r;
    line("decoder.uplayer" + std::to_string(i / nb + 1) + "." + std::to_string(i % nb),
         {{"fwd_cs_stream", r.fwd_cs_stream}, {"fwd_c2_stream", r.fwd_c2_stream}, {"fwd_stats_only", r.fwd_stats_only},
          {"fwd_join_conv1", r.fwd_join_conv1}, {"bwd_join_grad", r.bwd_join_grad}, {"bwd_join_stream", r.bwd_join_stream},
          {"bwd_fuse_c2", r.bwd_fuse_c2}, {"bwd_fuse_cs", r.bwd_fuse_cs}});
  }
  static const char* const kTail[] = {"GATHER", "JOIN", "STREAM", "UP5"};
  out += std::string("net: stem_fwd_stream=") + std::to_string(R.stem_fwd_stream) + " stem_bwd_fused=" + std::to_string(R.stem_bwd_fused) +
         " stem_dg_fused=" + std::to_string(R.stem_dg_fused) + " tail_fwd=" + kTail[R.tail_fwd] + " tail_bwd_fused=" + std::to_string(R.tail_bwd_fused) +
         " tail_wg_in_reduce=" + std::to_string(R.tail_wg_in_reduce) + " store8=" + std::to_string(R.store8) + "\n";
  return MMVAE_OK;
}

int Net::begin_pass(Pass& ps, int N, void* ws, size_t ws_bytes, const float* params, float* grads, float* bnbuf, long long* nbt, bool training) {
  const Plan& P = plan(N);
  if (P.route.refused) { set_error("%s", P.route.refused); return MMVAE_ERR_UNSUPPORTED; }
  if (ws_bytes < P.bytes) { set_error("workspace too small: %zu < %zu", ws_bytes, P.bytes); return MMVAE_ERR_WORKSPACE; }
  ps.P = &P; ps.base = static_cast<char*>(ws); ps.params = params; ps.grads = grads; ps.bnbuf = bnbuf; ps.nbt = nbt; ps.N = N;
  ps.training = training; ps.esz = esz();
  ps.part = reinterpret_cast<float*>(ps.base + P.partials);
  ps.wscratch = reinterpret_cast<float*>(ps.base + P.wscratch);
  return MMVAE_OK;
}

int Net::fill_consts(const Pass& ps, hipStream_t s) {
  float* c = reinterpret_cast<float*>(ps.base + ps.P->cvec);
  MM_TRY(launch_fill_f32(c, 1.f, 256, s));
  return launch_fill_f32(c + 256, 0.f, 256, s);
}

// ------------------------------------------------------------------------------------------------ conv helpers
// The pack that feeds a conv's FORWARD direction (down for Conv2d, up for ConvTranspose2d) is e4m3 bytes on an fp8 layer; every pack of an
// fp8 layer carries its weight scale.  Fragment-major or plain: settled per layer in settle_layout().
int Net::pack_down(const Pass& ps, const ConvW& w, hipStream_t s) {
  return op_pack_down(dt(), geom(w), ps.params + w.off, ps.packed(w.packD), s, w.wscale, (w.fp8 && !w.tr) ? 1 : 0, w.fragD);
}
int Net::pack_up(const Pass& ps, const ConvW& w, hipStream_t s) {
  return op_pack_up(dt(), geom(w), ps.params + w.off, ps.packed(w.packU), s, w.wscale, (w.fp8 && w.tr) ? 1 : 0, w.fragU);
}
// the second source and the layouts of the packed weights of a run_down / run_up launch (fwd: the launch is the layer's forward)
SecondSrc Net::second_src(const Pass& ps, const ConvW& w, bool fwd, bool frag, const ConvW* w2, const void* x2) const {
  SecondSrc q;
  if (w2) { q.x2 = x2; q.w2 = ps.packed(w2->packU); q.Cin2 = w2->D0; }
  q.fp8 = (w.fp8 && fwd) ? 1 : 0;
  q.wfrag = frag; q.wfrag2 = w2 ? w2->fragU : 0;
  return q;
}
static inline int small_size(const ConvW& w) { return conv_down_size(w.Hl, w.k, w.s, w.p); }
int Net::run_down(const Pass& ps, const ConvW& w, MapIn L, MapOut S, hipStream_t s, const ConvW* w2, const void* x2) {
  L.H = L.W = w.Hl; S.H = S.W = small_size(w);
  return op_run_down(dt(), dt(), geom(w), ps.packed(w.packD), L, S, ps.N, s, second_src(ps, w, !w.tr, w.fragD, w2, x2));   // fwd: a Conv2d's
}
int Net::run_up(const Pass& ps, const ConvW& w, MapIn S, MapOut L, hipStream_t s, const ConvW* w2, const void* x2) {
  S.H = S.W = small_size(w); L.H = L.W = w.Hl;
  return op_run_up(dt(), geom(w), ps.packed(w.packU), S, L, ps.N, s, second_src(ps, w, w.tr, w.fragU, w2, x2));            // fwd: a ConvTranspose2d's
}
hipStream_t Net::wgrad_stream(hipStream_t s) {
  if (side_state_ == 0) {
    side_state_ = 1;
    bool ok = hipStreamCreateWithFlags(&side_, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < kForkEvents && ok; ++i) ok = hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 16 && ok; ++i) ok = hipEventCreateWithFlags(&blk_ev_[i], hipEventDisableTiming) == hipSuccess;
    if (ok) ok = hipEventCreateWithFlags(&gram_ev_, hipEventDisableTiming) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); side_state_ = -1; }
  }
  return side_state_ == 1 ? side_ : s;
}
// kForkEvents > 2 x (forks + joins of one backward pass): no event is re-recorded while a wait on it may be pending
int Net::side_fork(hipStream_t s) {
  if (wgrad_stream(s) == s) return MMVAE_OK;
  hipEvent_t e = ev_[evi_++ % kForkEvents];
  bool ok = hipEventRecord(e, s) == hipSuccess && hipStreamWaitEvent(side_, e, 0) == hipSuccess;
  if (!ok) { set_error("side stream fork failed"); return MMVAE_ERR_HIP; }
  return MMVAE_OK;
}
int Net::side_join(hipStream_t s) {
  if (wgrad_stream(s) == s) return MMVAE_OK;
  hipEvent_t e = ev_[evi_++ % kForkEvents];
  bool ok = hipEventRecord(e, side_) == hipSuccess && hipStreamWaitEvent(s, e, 0) == hipSuccess;
  if (!ok) { set_error("side stream join failed"); return MMVAE_ERR_HIP; }
  return MMVAE_OK;
}

int Net::side_mark(int slot) {
  if (side_state_ != 1) return MMVAE_OK;
  bool ok = hipEventRecord(blk_ev_[slot & 15], side_) == hipSuccess;
  if (!ok) { set_error("side stream mark failed"); return MMVAE_ERR_HIP; }
  return MMVAE_OK;
}
int Net::side_wait_mark(int slot, hipStream_t s) {
  if (side_state_ != 1) return MMVAE_OK;
  bool ok = hipStreamWaitEvent(s, blk_ev_[slot & 15], 0) == hipSuccess;
  if (!ok) { set_error("side stream wait failed"); return MMVAE_ERR_HIP; }
  return MMVAE_OK;
}

int Net::run_wgrad(const Pass& ps, const ConvW& w, const BnSide& P, const BnSide& G, hipStream_t s, float* scratch, WgradReduceArgs* defer) {
  // (measured in round 3: a SECOND side stream with its own scratch, the weight gradients alternating between the two, is slower --
  // 7.74 vs 7.63 ms per step: the phases where the side stream lags are bandwidth-bound, two wgrad kernels at once only thrash)
  WgradOpts o;
  o.scratch = scratch ? scratch : ps.wscratch; o.scale = w.wscale; o.defer = defer;
  const int Hs = small_size(w);
  return op_run_wgrad(dt(), geom(w), MapIn(P, Hs, Hs), MapIn(G, w.Hl, w.Hl), ps.grads + w.off, ps.N, s, o);
}

int Net::reduce_wgrad_parts(const Pass& ps, const ConvW& w, const float* parts, int nparts, int ntaps, hipStream_t s) {
  return launch_wgrad_reduce(reduce_args(parts, nparts, ps.grads + w.off, w.D0, w.D1, ntaps, w.wscale), s);
}

// SyncBN: sum the partial rows locally, let the host's collective sum the row over the ranks (stream-ordered), and hand the
// finalize kernels that one row.  Two operand slots: the caller's stream and the side stream may both have one in flight.
int Net::sync_rows(const Pass& ps, const float* partials, int nparts, int width, hipStream_t s, float** out, int row_stride) {
  if (width > 1024) { set_error("sync_bn: %d statistics per BatchNorm > 1024", width); return MMVAE_ERR_UNSUPPORTED; }
  float* buf = reinterpret_cast<float*>(ps.base + ps.P->syncbuf) + (s == side_ ? 1024 : 0);
  MM_TRY(launch_partial_rowsum(partials, nparts, width, buf, s, row_stride));
  if (comm_) MM_TRY(comm_allreduce_sum((s == side_ && comm_side_) ? comm_side_ : comm_, buf, width, s));
  else if (ar_fn_(buf, width, s, ar_user_) != 0) { set_error("sync_bn: the all-reduce callback failed"); return MMVAE_ERR_ARG; }
  *out = buf;
  return MMVAE_OK;
}

int Net::bn_fwd(const Pass& ps, const Bn& bn, int nparts, double count, hipStream_t s, long part_off, float in_scale) {
  if (!ps.training) {      // fold_bn_eval() has written every (scale, shift) pair of the entry point already
    if (eval_folded_) return MMVAE_OK;
    set_error("bn_eval: the entry point did not fold its BatchNorms"); return MMVAE_ERR_ARG;
  }
  BnFinalizeArgs a;
  a.in_scale = in_scale;
  a.partials = ps.part + part_off; a.nparts = nparts; a.C = bn.C; a.count = count;
  if (sync_bn_on()) {      // statistics over the global batch (equal shards per rank)
    float* row = nullptr;
    MM_TRY(sync_rows(ps, a.partials, nparts, 2 * bn.C, s, &row));
    a.partials = row; a.nparts = 1; a.count = count * ar_world_;
  }
  a.gamma = ps.params + bn.g_off; a.beta = ps.params + bn.b_off;
  a.running_mean = ps.bnbuf ? ps.bnbuf + bn.rm_off : nullptr; a.running_var = ps.bnbuf ? ps.bnbuf + bn.rv_off : nullptr;
  a.nbt = ps.nbt ? ps.nbt + bn.nbt_idx : nullptr;
  const BnRows r = ps.rows(bn);
  a.mean = r.mean; a.istd = r.istd; a.scale = r.scale; a.shift = r.shift;
  a.momentum = 0.1f; a.eps = 1e-5f;
  return launch_bn_finalize(a, s);
}

int Net::fold_bn_eval(const Pass& ps, int which, hipStream_t s) {
  std::vector<BnFoldEntry> tab;
  auto add = [&](const Bn& bn, float in_scale) {
    BnFoldEntry e;
    e.g_off = (int)bn.g_off; e.b_off = (int)bn.b_off; e.rm_off = (int)bn.rm_off; e.rv_off = (int)bn.rv_off;
    e.scale_off = (int)bn.row(Bn::SCALE); e.shift_off = (int)bn.row(Bn::SHIFT); e.C = bn.C; e.in_scale = in_scale;
    tab.push_back(e);
  };
  if (which == 0) add(bn0, 1.f); else add(dbn0, dstem.wscale);
  for (const Block& B : which == 0 ? enc : dec) {
    add(B.b1, B.c1.wscale); add(B.b2, B.c2.wscale);
    if (!B.identity) add(B.bs, B.cs.wscale);
  }
  if (which == 1) add(bn_out, 1.f);
  MM_TRY(launch_bn_fold_eval(tab.data(), (int)tab.size(), ps.params, ps.bnbuf, reinterpret_cast<float*>(ps.base + ps.P->bnws), 1e-5f, s));
  eval_folded_ = true;
  return MMVAE_OK;
}

BnBwdFinalizeArgs Net::bwd_finalize_args(const Pass& ps, const Bn& bn, const float* partials, int nparts, int ny, int which,
                                         double count) const {
  const BnRows r = ps.rows(bn);
  BnBwdFinalizeArgs a;
  a.partials = partials; a.nparts = nparts; a.C = bn.C; a.which = which; a.ny = ny;
  a.count = count; a.gamma = ps.params + bn.g_off; a.mean = r.mean; a.istd = r.istd;
  a.dgamma = ps.grads + bn.g_off; a.dbeta = ps.grads + bn.b_off;
  a.coefA = r.A; a.coefB = r.B; a.coefC = r.C;
  return a;
}
// SyncBN backward: dgamma / dbeta stay the rank's own sums (the gradient all-reduce adds the ranks up), the coefficients of
// dx = A*g + B*y + C use the sums over the global batch -- so the local finalize runs first and a second one, fed with the
// all-reduced row, overwrites the coefficients.
int Net::bn_backward_coefs(const Pass& ps, const Bn& bn, int nparts, int ny, int which, double count, hipStream_t s, float* dbias_conv) {
  BnBwdFinalizeArgs l = bwd_finalize_args(ps, bn, ps.part, nparts, ny, which, count);
  if (!sync_bn_on()) l.dbias_conv = dbias_conv;
  MM_TRY(launch_bn_bwd_finalize(l, s));
  if (!sync_bn_on()) return MMVAE_OK;
  float* row = nullptr;
  MM_TRY(sync_rows(ps, ps.part, nparts, (1 + ny) * bn.C, s, &row));
  BnBwdFinalizeArgs g = bwd_finalize_args(ps, bn, row, 1, ny, which, count * ar_world_);
  g.dgamma = nullptr; g.dbeta = nullptr;
  // the gradient all-reduce sums the ranks: every rank contributes 1/world of the global closed form
  g.dbias_conv = dbias_conv; g.dbias_scale = 1.f / (float)ar_world_;
  return launch_bn_bwd_finalize(g, s);
}
// the two BatchNorms of a residual join (partials rows: sum g, sum g*y2, sum g*ys) in one launch
int Net::bn_backward_coefs_join(const Pass& ps, const Bn& b2, const Bn& bs, int nparts, double count, hipStream_t s) {
  MM_TRY(launch_bn_bwd_finalize2(bwd_finalize_args(ps, b2, ps.part, nparts, 2, 0, count),
                                 bwd_finalize_args(ps, bs, ps.part, nparts, 2, 1, count), s));
  if (!sync_bn_on()) return MMVAE_OK;
  float* row = nullptr;
  MM_TRY(sync_rows(ps, ps.part, nparts, 3 * b2.C, s, &row));
  BnBwdFinalizeArgs g2 = bwd_finalize_args(ps, b2, row, 1, 2, 0, count * ar_world_);
  BnBwdFinalizeArgs gs = bwd_finalize_args(ps, bs, row, 1, 2, 1, count * ar_world_);
  g2.dgamma = g2.dbeta = gs.dgamma = gs.dbeta = nullptr;
  return launch_bn_bwd_finalize2(g2, gs, s);
}
int Net::bn_relu_backward(const Pass& ps, const Bn& bn, const void* g, const void* y, void* dy, long npix, hipStream_t s, int nparts_ready) {
  const BnSide a = ps.rows(bn).side(y);
  const int np = nparts_ready > 0 ? nparts_ready : launch_bn_bwd_reduce(dt(), g, nullptr, a, BnSide{}, ps.part, npix, bn.C, s);
  MM_TRY(np);
  MM_TRY(bn_backward_coefs(ps, bn, np, 1, 0, (double)npix, s));
  return launch_bn_bwd_apply(dt(), g, nullptr, a, BnSide{}, dy, nullptr, npix, bn.C, s);
}
int Net::join_backward(const Pass& ps, const Block& B, const BnSide& sc, const void* g, bool g_masked, void* dy2, void* dys, hipStream_t s,
                       int nparts_ready) {
  const BnSide s2 = ps.rows(B.b2).side(ps.base + B.y2);
  const long npix = (long)ps.N * B.Hout * B.Wout;
  // g_masked: plain sums, no forward rows; else the reduce applies the join's ReLU mask itself
  const int np = nparts_ready > 0 ? nparts_ready
                 : g_masked       ? launch_bn_bwd_reduce(dt(), g, nullptr, BnSide{s2.y}, BnSide{sc.y}, ps.part, npix, B.C, s)
                                  : launch_bn_bwd_reduce(dt(), g, nullptr, s2, sc, ps.part, npix, B.C, s);
  MM_TRY(np);
  if (B.identity) MM_TRY(bn_backward_coefs(ps, B.b2, np, 2, 0, (double)npix, s));
  else MM_TRY(bn_backward_coefs_join(ps, B.b2, B.bs, np, (double)npix, s));
  if (!dy2) return MMVAE_OK;
  return launch_bn_bwd_apply(dt(), g, nullptr, s2, sc, dy2, dys, npix, B.C, s);
}

// ------------------------------------------------------------------------------------------------ weight re-packs per entry point
// (recorded by launch_pack() while a batch is open; see pack_batch_begin/flush)
int Net::packs_enc_fwd(const Pass& ps, hipStream_t s) {
  MM_TRY(op_pack_stem(dt(), ps.params + stem.off, cfg.in_ch, ps.packed(stem_pack), s));
  for (const Block& B : enc) {
    MM_TRY(pack_down(ps, B.c1, s));
    MM_TRY(pack_down(ps, B.c2, s));
    if (!B.identity) MM_TRY(pack_down(ps, B.cs, s));
  }
  const int nt = Hf * Wf;
  for (int h = 0; h < (cfg.need_logvar ? 2 : 1); ++h) {
    const ConvW& hw = h == 0 ? head_mu : head_lv;
    const long poff = h == 0 ? head_pack_mu : head_pack_lv;
    PackArgs pa; std::memset(&pa, 0, sizeof(pa));
    pa.src = ps.params + hw.off; pa.dst = ps.packed(poff);
    pa.cols = cfg.z; pa.K = 256; pa.ntaps = nt; pa.s_col = 256; pa.s_k = 1; pa.scale = 1.0f / nt;
    MM_TRY(launch_pack(dt(), pa, s));
  }
  return MMVAE_OK;
}

int Net::packs_enc_bwd(const Pass& ps, hipStream_t s) {
  const int Ch = cfg.need_logvar ? 2 * cfg.z : cfg.z;
  PackArgs pa; std::memset(&pa, 0, sizeof(pa));
  pa.src = ps.params + head_mu.off; pa.dst = ps.packed(head_pack_dg);
  pa.cols = 256; pa.K = Ch; pa.ntaps = 1; pa.s_col = 1; pa.s_k = 256; pa.scale = 1.0f / (Hf * Wf);
  MM_TRY(launch_pack(dt(), pa, s));
  for (const Block& B : enc) {
    MM_TRY(pack_up(ps, B.c2, s));
    MM_TRY(pack_up(ps, B.c1, s));
    if (!B.identity) MM_TRY(pack_up(ps, B.cs, s));
  }
  if (const ConvW& w = enc[0].c2; enc[0].r.bwd_c2_dgrad_stream)      // its data gradient as a forward 3x3 conv over dy
    MM_TRY(op_pack_flipped3(dt(), ps.params + w.off, ps.packed(l1c2_flip), 32, 32, s, w.wscale));
  return MMVAE_OK;
}

int Net::packs_dec_fwd(const Pass& ps, hipStream_t s) {
  MM_TRY(pack_up(ps, dstem, s));
  for (const Block& B : dec) {
    MM_TRY(pack_down(ps, B.c1, s));
    if (B.identity) MM_TRY(pack_down(ps, B.c2, s));       // 3x3 Conv2d
    else { MM_TRY(pack_up(ps, B.c2, s)); MM_TRY(pack_up(ps, B.cs, s)); }
  }
  PackArgs pa; std::memset(&pa, 0, sizeof(pa));
  pa.src = ps.params + tail.off; pa.dst = ps.packed(tail_pack_f);
  pa.cols = 16; pa.cols_valid = cfg.out_ch; pa.K = 16; pa.ntaps = 9; pa.s_col = 144; pa.s_k = 9; pa.scale = 1.f;
  for (int t = 0; t < 9; ++t) pa.tap_off[t] = t;
  MM_TRY(launch_pack(dt(), pa, s));
  return MMVAE_OK;
}

int Net::packs_dec_bwd(const Pass& ps, bool need_denc, hipStream_t s) {
  PackArgs pa; std::memset(&pa, 0, sizeof(pa));
  pa.src = ps.params + tail.off; pa.dst = ps.packed(tail_pack_d);
  pa.cols = 16; pa.K = 8; pa.K_valid = cfg.out_ch; pa.ntaps = 9; pa.s_col = 9; pa.s_k = 144; pa.scale = 1.f;
  for (int t = 0; t < 9; ++t) pa.tap_off[t] = t;
  MM_TRY(launch_pack(dt(), pa, s));
  for (const Block& B : dec) {
    MM_TRY(pack_up(ps, B.c1, s));
    if (B.identity) MM_TRY(pack_up(ps, B.c2, s));
    else { MM_TRY(pack_down(ps, B.c2, s)); MM_TRY(pack_down(ps, B.cs, s)); }
  }
  if (need_denc) MM_TRY(pack_down(ps, dstem, s));
  return MMVAE_OK;
}

// ------------------------------------------------------------------------------------------------ encoder
int Net::stage_labels(int N, const void* labels, int label_bytes, float mean, float stdv, float* image, void* ws, size_t ws_bytes, hipStream_t s) {
  Pass ps;
  MM_TRY(begin_pass(ps, N, ws, ws_bytes));
  return launch_normalise(dt(), labels, label_bytes, (long)N * cfg.in_ch * cfg.S * cfg.S, mean, stdv, ps.base + ps.P->x_t, image, s);
}

int Net::encoder_fwd(int N, const float* x, const float* params, float* bnbuf, long long* nbt, void* ws, size_t ws_bytes,
                     float* mu, float* logvar, int training, hipStream_t s, bool staged) {
  if (Hf > 2) { set_error("encoder: image size %d unsupported (final map %dx%d)", cfg.S, Hf, Wf); return MMVAE_ERR_UNSUPPORTED; }
  Pass ps;
  MM_TRY(begin_pass(ps, N, ws, ws_bytes, params, nullptr, bnbuf, nbt, training != 0));
  const Plan& P = *ps.P;
  char* const base = ps.base;
  float* const part = ps.part;
  float* stats = training ? part : nullptr;
  const int S = cfg.S;
  pack_batch_begin();                       // every weight re-pack of this entry point in ONE launch
  MM_TRY(packs_enc_fwd(ps, s));
  MM_TRY(pack_batch_flush(dt(), s));
  eval_folded_ = false;
  gram_ready_ = false; gram_fwd_N_ = training ? N : 0; gram_fwd_ws_ = ws;
  if (!training) MM_TRY(fold_bn_eval(ps, 0, s));
  if (!staged) MM_TRY(launch_convert(DT_F32, dt(), x, base + P.x_t, (long)N * cfg.in_ch * S * S, s));
  int np;
  if (P.route.stem_fwd_stream) {
    np = launch_stem_fwd_stream(dt(), base + P.x_t, params + stem.off, base + P.y0, stats, N, S, s);
  } else {
    // stem Conv2d(in_channels -> 32, k5 s2 p2) (model.py:94): the planar image (in_channels <= 4 planes) is staged as a zero-padded
    // VE-channel NHWC patch in LDS and runs through the MFMA patch-tile kernel; BatchNorm statistics come out of its epilogue.
    np = op_run_stem(dt(), ps.packed(stem_pack), base + P.x_t, cfg.in_ch, S, MapOut(base + P.y0, H1, W1, stats), N, s);
  }
  MM_TRY(np);
  MM_TRY(bn_fwd(ps, bn0, np, (double)N * H1 * W1, s));
  BnSide in{base + P.y0, ps.rows(bn0).affine()};      // the block input under its prologue (the stem's BatchNorm + ReLU; none behind a join)
  if (cfg.blocks > 1) MM_TRY(fill_consts(ps, s));
  for (size_t i = 0; i < enc.size(); ++i) {
    Block& B = enc[i];
    const double cnt = (double)N * B.Hout * B.Wout;
    const BnSide s1 = ps.rows(B.b1).side(base + B.y1), s2 = ps.rows(B.b2).side(base + B.y2), sc = ps.shortcut(B, in);
    float* const stats_sc = stats ? stats + kPartialFloats : nullptr;
    // shortcut branch (conv + its BatchNorm) on the side stream, concurrently with conv1 -> bn1 -> conv2 -> bn2 -- unless one kernel takes conv1 with it
    const bool stream1 = B.r.fwd_c1_cs_stream, stream2 = B.r.fwd_c2_stream, fork = !B.identity && !stream1;
    if (stream1) {
      np = launch_conv3_stream(dt(), 2, MapIn(in, B.Hin, B.Win), ps.packed(B.c1.packD), ps.packed(B.cs.packD),
                               MapOut(base + B.y1, B.Hout, B.Wout, stats), MapOut(base + B.ys, B.Hout, B.Wout, stats_sc), N, s);
      MM_TRY(np);
      MM_TRY(bn_fwd(ps, B.bs, np, cnt, s, kPartialFloats, B.cs.wscale));
      MM_TRY(bn_fwd(ps, B.b1, np, cnt, s, 0, B.c1.wscale));
    } else if (!B.identity) {
      if (fork) MM_TRY(side_fork(s));
      hipStream_t ss = fork ? wgrad_stream(s) : s;
      np = run_down(ps, B.cs, in, MapOut(base + B.ys, stats_sc), ss);
      MM_TRY(np);
      MM_TRY(bn_fwd(ps, B.bs, np, cnt, ss, kPartialFloats, B.cs.wscale));
    }
    if (!stream1) {
      np = run_down(ps, B.c1, in, MapOut(base + B.y1, stats), s);
      MM_TRY(np);
      MM_TRY(bn_fwd(ps, B.b1, np, cnt, s, 0, B.c1.wscale));
    }
    if (stream2)
      np = launch_conv3_stream(dt(), 1, MapIn(s1, B.Hout, B.Wout), ps.packed(B.c2.packD), nullptr, MapOut(base + B.y2, B.Hout, B.Wout, stats),
                               MapOut(), N, s);
    else
      np = run_down(ps, B.c2, s1, MapOut(base + B.y2, stats), s);
    MM_TRY(np);
    MM_TRY(bn_fwd(ps, B.b2, np, cnt, s, 0, B.c2.wscale));
    if (fork) MM_TRY(side_join(s));
    MM_TRY(launch_join_fwd(dt(), s2, sc, base + B.out, (long)N * B.Hout * B.Wout, B.C, s));
    in = BnSide{base + B.out};
  }
  // global average pool + the two 1x1 heads (model.py:123-128) as ONE k=Hf,s=Hf conv whose taps share W/(Hf*Wf)
  for (int h = 0; h < (cfg.need_logvar ? 2 : 1); ++h) {
    const ConvW& hw = h == 0 ? head_mu : head_lv;
    const MapOut latent(h == 0 ? mu : logvar, 1, 1);      // f32 [N][1][1][z]
    MM_TRY(op_run_down(dt(), DT_F32, ConvGeom{hw.D0, hw.D1, Hf, Hf, 0}, ps.packed(h == 0 ? head_pack_mu : head_pack_lv), MapIn(in.y, Hf, Wf), latent, N, s));
  }
  return MMVAE_OK;
}

int Net::encoder_bwd(int N, const float* d_mu, const float* d_logvar, const float* params, float* grads, void* ws, size_t ws_bytes,
                     hipStream_t s) {
  Pass ps;
  MM_TRY(begin_pass(ps, N, ws, ws_bytes, params, grads));
  const Plan& P = *ps.P;
  char* const base = ps.base;
  float* const part = ps.part;
  const NetRoute& R = P.route;
  const BnRows r0 = ps.rows(bn0);
  const int Ch = cfg.need_logvar ? 2 * cfg.z : cfg.z;
  const int nt = Hf * Wf;
  pack_batch_begin();
  MM_TRY(packs_enc_bwd(ps, s));
  MM_TRY(pack_batch_flush(dt(), s));
  // ---- heads: dh = [d_mu | d_logvar] in T
  MM_TRY(launch_concat2_to_t(dt(), d_mu, cfg.need_logvar ? d_logvar : nullptr, N, cfg.z, cfg.need_logvar ? cfg.z : 0, base + P.dh, s));
  {
    // both heads' weight gradient as the k=Hf,s=Hf conv's, every tap adding into the one 1x1 weight (the average pool)
    WgradArgs a;
    wgrad_args(a, ConvGeom{Ch, 256, Hf, Hf, 0}, N, MapIn(base + P.dh, 1, 1), MapIn(base + enc.back().out, Hf, Wf), grads + head_mu.off, ps.wscratch,
               1.0f / nt);
    a.sA = 256; a.sB = 1; std::fill_n(a.tap_off, nt, 0);
    MM_TRY(side_fork(s));
    MM_TRY(launch_wgrad(dt(), a, wgrad_stream(s)));
    // the stem's input-only work (patch gram matrix / im2col) early, off the tail of the critical path
    if (R.stem_bwd_fused && !(gram_ready_ && gram_fwd_N_ == N && gram_fwd_ws_ == ws)) {
      MM_TRY(launch_stem_gram(dt(), base + P.x_t, reinterpret_cast<float*>(base + P.stem_gram), 1024L * stem_bwd_part_floats(),
                              reinterpret_cast<double*>(base + P.stem_R), N, cfg.S, H1, W1, wgrad_stream(s)));
      // the stem's finalize at the very end waits for THIS, not for the whole side stream (whose last weight gradients may still run)
      if (side_state_ == 1 && hipEventRecord(gram_ev_, side_) != hipSuccess) { set_error("side stream mark failed"); return MMVAE_ERR_HIP; }
    }
    gram_ready_ = false;            // (consumed: the next backward pass belongs to another forward pass)
    if (!R.stem_bwd_fused && cfg.in_ch == 1 && wgrad_stream(s) != s) MM_TRY(launch_stem_im2col(dt(), base + P.x_t, base + P.col, N, cfg.S, cfg.S, H1, W1, wgrad_stream(s)));
    GatherArgs g; std::memset(&g, 0, sizeof(g));
    g.x = base + P.dh; g.w = ps.packed(head_pack_dg); g.y = base + P.g[0];
    g.N = N; g.Hi = 1; g.Wi = 1; g.Cin = Ch; g.Ho = Hf; g.Wo = Wf; g.Cout = 256; g.SI = 1; g.SO = Hf;
    g.nphase = nt;
    for (int i = 0; i < nt; ++i) { g.phases[i] = Phase{i / Wf, i % Wf, 1, 1, 1, i, 0}; g.taps[i] = Tap{0, 0}; }
    MM_TRY(launch_gather_gemm(dt(), dt(), g, s));
  }
  int cur = 0;   // d_out lives in g[cur]
  long stem_dy1 = 0, stem_dys = 0;   // workspace offsets of layer1's dy1 / dys, for the stem's fused backward
  const int ne = (int)enc.size();
  for (int i = ne - 1; i >= 0; --i) {
    Block& B = enc[i];
    const long npix = (long)N * B.Hout * B.Wout;
    const BnSide in = i == 0 ? BnSide{base + P.y0, r0.affine()} : BnSide{base + enc[i - 1].out};      // the block input under its prologue
    const BnSide s1 = ps.rows(B.b1).side(base + B.y1), sc = ps.shortcut(B, in);
    // dy1 / dy2 / dys alternate between two sets, so this block only has to wait for the weight gradients of the block
    // before the previous one (the side stream may lag one block behind)
    // The two blocks visited first (small tensors) own private sets: with a deferred decoder join the side stream may still be
    // reading the shared sets for the decoder's weight gradients when they start.  The third block waits for the first one's
    // mark, which -- the side stream being in order -- also covers everything the decoder left there.
    const int ds = i & 1;
    const bool priv = i >= ne - 2;
    const long dy1o = priv ? P.edy1[i - (ne - 2)] : P.dy1[ds], dy2o = priv ? P.edy2[i - (ne - 2)] : P.dy2[ds];
    // an identity shortcut's gradient is the masked incoming gradient itself: it goes straight into the block-input gradient
    const long dyso = B.identity ? P.g[cur ^ 1] : (priv ? P.edys[i - (ne - 2)] : P.dys[ds]);
    if (i + 2 <= ne - 1) MM_TRY(side_wait_mark(i + 2, s));
    // join backward: g = d_out * [out > 0] feeds bn2 (y2) and the shortcut BN (ys)
    MM_TRY(join_backward(ps, B, sc, base + P.g[cur], false, base + dy2o, base + dyso, s));
    // conv2 (3x3 s1): wgrad with a1 = relu(bn1(y1)) recomputed in the load prologue; dgrad -> d_a1
    hipStream_t wsm = wgrad_stream(s);
    MM_TRY(side_fork(s));
    // (measured and not kept: a THIRD stream for this block's two weight-gradient kernels, so that they need not wait for the side stream's
    // backlog of deeper layers -- 6.93-6.96 against 6.96 ms per step, within the run-to-run spread)
    // encoder.layer1 (the block the step ends on): conv2's partial images go to the second scratch (idle in this pass) and are reduced
    // AFTER the block's other weight gradient has been enqueued -- under the stem backward's load a 19 MB reduce takes 120 us instead of
    // 10, and it sat in front of the last big kernel of the side stream
    WgradReduceArgs late; late.nparts = 0;
    const void *const dy1 = base + dy1o, *const dy2 = base + dy2o, *const dys = base + dyso;
    if (B.r.bwd_c2_late_reduce && wsm != s)
      MM_TRY(run_wgrad(ps, B.c2, BnSide{dy2}, s1, wsm, reinterpret_cast<float*>(base + P.wscratch2), &late));
    else
      MM_TRY(run_wgrad(ps, B.c2, BnSide{dy2}, s1, wsm));
    const bool pair = B.r.bwd_pair_wgrad;     // (encoder.layer1: the shortcut's weight gradient rides on conv1's pass over the block input, below)
    if (!B.identity && !pair) MM_TRY(run_wgrad(ps, B.cs, BnSide{dys}, in, wsm));
    int np1 = 0;                         // rows of bn1's backward sums when the data-gradient pass has left them in `part`
    if (B.r.bwd_c2_dgrad_stream) {
      // encoder.layer1.conv2: the data gradient as a per-wave stream over dy2 (conv3_stream_kernel) with bn1's backward sums from the same pass
      np1 = launch_conv3_stream_bwd(dt(), MapIn(dy2, B.Hout, B.Wout), ps.packed(l1c2_flip), s1, MapOut(base + P.da1, B.Hout, B.Wout, part), N, s);
      MM_TRY(np1);
    } else
      MM_TRY(run_up(ps, B.c2, dy2, base + P.da1, s));
    MM_TRY(bn_relu_backward(ps, B.b1, base + P.da1, base + B.y1, base + dy1o, npix, s, np1));      // bn1 + relu backward
    // conv1 (3x3) and the 1x1 s2 shortcut: weight gradients, then d_xin = dgrad(conv1) + dgrad(shortcut)
    MM_TRY(side_fork(s));
    int taken = 0;
    if (pair) {
      WgradOpts o;
      o.scratch = ps.wscratch; o.scale = B.c1.wscale; o.scale2 = B.cs.wscale;
      taken = op_run_wgrad_pair(dt(), geom(B.c1), geom(B.cs), MapIn(dy1, B.Hout, B.Wout), dys, MapIn(in, B.Hin, B.Win), grads + B.c1.off,
                                grads + B.cs.off, N, wsm, o);
      MM_TRY(taken);
      if (!taken) MM_TRY(run_wgrad(ps, B.cs, BnSide{dys}, in, wsm));
    }
    if (!taken) MM_TRY(run_wgrad(ps, B.c1, BnSide{dy1}, in, wsm));
    if (late.nparts > 0) MM_TRY(launch_wgrad_reduce(late, wsm));
    MM_TRY(side_mark(i));
    if (i == 0 && R.stem_dg_fused) {
      // the gradient of the stem's output is never a tensor: stem_bwd_kernel<DG> recomputes it row by row from dy1 / dys (below)
      stem_dy1 = dy1o; stem_dys = dyso;
    } else if (B.identity)     // d_xin already holds the shortcut's share: the main path's data gradient is added to it
      MM_TRY(run_up(ps, B.c1, dy1, MapOut::add(base + P.g[cur ^ 1]), s));
    else                // one kernel: the 1x1 stride-2 shortcut's data gradient is a second source of the 3x3 conv's (phase (0,0))
      MM_TRY(run_up(ps, B.c1, dy1, base + P.g[cur ^ 1], s, &B.cs, dys));
    cur ^= 1;
  }
  // ---- stem: bn0 + relu backward and the 5x5 weight gradient
  if (R.stem_bwd_fused) {
    // one pass over g and y0 (stem_bwd.hip): BatchNorm sums and the three pixel reductions dW is an affine function of; no dy
    // tensor, no im2col, nothing waits on a grid-wide reduction except the 32-block finalize
    const long npix = (long)N * H1 * W1;
    const Block& B0 = enc[0];
    const int np = R.stem_dg_fused
        ? launch_stem_bwd_dg(base + stem_dy1, base + stem_dys, ps.packed(B0.c1.packU), ps.packed(B0.cs.packU), base + P.y0, base + P.x_t,
                             r0.scale, r0.shift, part, kPartialFloats, N, cfg.S, H1, W1, s)
        : launch_stem_bwd(dt(), base + P.g[cur], base + P.y0, base + P.x_t, r0.scale, r0.shift, part, kPartialFloats, N, cfg.S, H1, W1, s);
    MM_TRY(np);
    const float* gsum = nullptr; double cnt = (double)npix;
    if (sync_bn_on()) {
      float* row = nullptr;
      MM_TRY(sync_rows(ps, part, np, 64, s, &row, stem_bwd_part_floats()));
      gsum = row; cnt *= ar_world_;
    }
    if (side_state_ == 1 && hipStreamWaitEvent(s, gram_ev_, 0) != hipSuccess) { set_error("side stream wait failed"); return MMVAE_ERR_HIP; }
    MM_TRY(launch_stem_bwd_finalize(part, np, reinterpret_cast<const double*>(base + P.stem_R), params + stem.off, gsum, cnt,
                                    params + bn0.g_off, r0.mean, r0.istd, grads + bn0.g_off, grads + bn0.b_off, grads + stem.off, s));
    return side_join(s);             // every weight gradient of this pass
  }
  // ---- stem: bn0 + relu backward, then the 5x5 weight gradient
  MM_TRY(side_wait_mark(1, s));    // the stem uses dy set 1 (block index -1): block 1's weight gradients read it last
  MM_TRY(bn_relu_backward(ps, bn0, base + P.g[cur], base + P.y0, base + P.dy1[1], (long)N * H1 * W1, s));
  MM_TRY(side_fork(s));
  hipStream_t wsm = wgrad_stream(s);
  const MapIn dy(base + P.dy1[1], H1, W1);
  WgradArgs a;
  if (cfg.in_ch > 1) {
    // in_channels > 1 (main.py:555): G = the image as NHWC with 16 zero-padded channels, the generic 25-tap weight gradient
    MM_TRY(launch_planar_to_nhwc16(dt(), static_cast<const void*>(base + P.x_t), dt(), base + P.col, N, cfg.in_ch, cfg.S * cfg.S, wsm));
    wgrad_args(a, ConvGeom{32, 16, 5, 2, 2}, N, dy, MapIn(base + P.col, cfg.S, cfg.S), grads + stem.off, ps.wscratch);
    a.Cb_valid = cfg.in_ch; a.sA = 25 * cfg.in_ch;
  } else {
    // im2col of the 1-channel image (25 taps padded to 32 columns) + the MFMA weight-gradient kernel as a 1x1 conv
    if (wsm == s) MM_TRY(launch_stem_im2col(dt(), base + P.x_t, base + P.col, N, cfg.S, cfg.S, H1, W1, wsm));   // else: done early
    wgrad_args(a, ConvGeom{32, 32, 1, 1, 0}, N, dy, MapIn(base + P.col, H1, W1), grads + stem.off, ps.wscratch);
    a.Cb_valid = 25; a.sA = 25;
  }
  MM_TRY(launch_wgrad(dt(), a, wsm));
  return side_join(s);
}

// ------------------------------------------------------------------------------------------------ decoder
int Net::decoder_fwd(int N, const float* encv, const float* params, float* bnbuf, long long* nbt, void* ws, size_t ws_bytes,
                     float* recon, int training, hipStream_t s) {
  Pass ps;
  MM_TRY(begin_pass(ps, N, ws, ws_bytes, params, nullptr, bnbuf, nbt, training != 0));
  const Plan& P = *ps.P;
  char* const base = ps.base;
  float* const part = ps.part;
  float* stats = training ? part : nullptr;
  const NetRoute& R = P.route;
  pack_batch_begin();
  MM_TRY(packs_dec_fwd(ps, s));
  MM_TRY(pack_batch_flush(dt(), s));
  eval_folded_ = false;
  if (!training) MM_TRY(fold_bn_eval(ps, 1, s));
  MM_TRY(launch_convert(DT_F32, dt(), encv, base + P.enc_t, (long)N * cfg.z, s));
  // stem ConvTranspose2d(z -> 128, k2) on the 1x1 latent (model.py:159-161,182)
  int np = run_up(ps, dstem, base + P.enc_t, MapOut(base + P.y0d, stats), s);
  MM_TRY(np);
  MM_TRY(bn_fwd(ps, dbn0, np, (double)N * 4, s, 0, dstem.wscale));
  BnSide in{base + P.y0d, ps.rows(dbn0).affine()};      // the block input under its prologue (see encoder_fwd)
  const int nd = (int)dec.size();
  if (cfg.blocks > 1) {
    // the first block of a deeper decoder has an identity shortcut: it needs the stem's activation as a tensor
    MM_TRY(fill_consts(ps, s));
    MM_TRY(launch_affine_act(dt(), in, 1, base + P.act0d, (long)N * 4, 128, s));
    in = BnSide{base + P.act0d};
  }
  int c1_done = 0;                 // rows of bn1 statistics the previous block's join kernel left for this block's conv1 (0: conv1 not done)
  for (int i = 0; i < nd; ++i) {
    Block& B = dec[i];
    const double cnt = (double)N * B.Hout * B.Wout;
    const BnSide s1 = ps.rows(B.b1).side(base + B.y1), s2 = ps.rows(B.b2).side(base + B.y2), sc = ps.shortcut(B, in);
    // a ConvTranspose2d forward: the per-wave stream (conv_fstream.hip) where routed -- on the up5 route statistics only, nothing in eval mode -- else the up conv
    auto convT = [&](const ConvW& w, bool stream, const BnSide& x, long y, float* st, hipStream_t q) {
      const bool stats_only = B.r.fwd_stats_only;
      if (stats_only && !st) return 1;
      if (stream) return launch_convT4_stream(dt(), MapIn(x, B.Hin, B.Win), ps.packed(w.packU), MapOut(stats_only ? nullptr : base + y, B.Hout, B.Wout, st),
                                              N, q, (R.store8 && i == nd - 1) ? 1 : 0);
      return run_up(ps, w, x, MapOut(base + y, st), q);
    };
    // upsample (shortcut) branch on the side stream, concurrently with conv1 -> bn1 -> conv2 -> bn2
    if (!B.identity) {
      MM_TRY(side_fork(s));
      hipStream_t ss = wgrad_stream(s);
      np = convT(B.cs, B.r.fwd_cs_stream, in, B.ys, stats ? stats + kPartialFloats : nullptr, ss);
      MM_TRY(np);
      MM_TRY(bn_fwd(ps, B.bs, np, cnt, ss, kPartialFloats, B.cs.wscale));
    }
    // (conv1 already done: the previous block's join kernel computed it from the joined row it had in LDS -- join_conv1_fwd below)
    np = c1_done > 0 ? c1_done : run_down(ps, B.c1, in, MapOut(base + B.y1, stats), s);
    c1_done = 0;
    MM_TRY(np);
    MM_TRY(bn_fwd(ps, B.b1, np, (double)N * B.Hin * B.Win, s, 0, B.c1.wscale));
    if (B.identity)    // 3x3 Conv2d, shape preserving
      np = run_down(ps, B.c2, s1, MapOut(base + B.y2, stats), s);
    else
      np = convT(B.c2, B.r.fwd_c2_stream, s1, B.y2, stats, s);
    MM_TRY(np);
    MM_TRY(bn_fwd(ps, B.b2, np, cnt, s, 0, B.c2.wscale));
    if (!B.identity) MM_TRY(side_join(s));
    if (i == nd - 1 && R.tail_fwd != TAIL_GATHER) break;     // the join of the last block happens inside the tail conv kernel
    if (B.r.fwd_join_conv1) {      // the join computes the next block's conv1 and bn1's statistics as well
      c1_done = launch_join_conv1_fwd(s2, sc, ps.packed(dec[i + 1].c1.packD), base + B.out, base + dec[i + 1].y1, stats, B.C,
                                      (long)N * B.Hout * B.Wout, s);
      MM_TRY(c1_done);
    } else
    MM_TRY(launch_join_fwd(dt(), s2, sc, base + B.out, (long)N * B.Hout * B.Wout, B.C, s));
    in = BnSide{base + B.out};
  }
  // tail conv (+bias) and the output BatchNorm (model.py:193)
  float* r_raw = reinterpret_cast<float*>(base + P.r_raw);
  if (R.tail_fwd != TAIL_GATHER) {
    const Block& B = dec.back();     // (the join left to this kernel: `in` is still the block's input)
    const BnSide s1 = ps.rows(B.b1).side(base + B.y1), s2 = ps.rows(B.b2).side(base + B.y2), sc = ps.shortcut(B, in);
    if (R.tail_fwd == TAIL_UP5)
      // the join + tail conv with both branch outputs recomputed from the ConvTranspose2d inputs (0.34 GB) instead of read back (1.34 GB),
      // and (training) stored from here for the backward pass
      np = launch_up5_tail_fwd(s1, ps.packed(B.c2.packU), in, ps.packed(B.cs.packU), s2.fwd, sc.fwd, params + tail.off,
                               params + tail_bias, r_raw, stats, N, s, stats ? base + B.y2 : nullptr, stats ? base + B.ys : nullptr);
    else if (R.tail_fwd == TAIL_STREAM)
      np = launch_tail_fwd_stream(dt(), s2, sc, params + tail.off, params + tail_bias, r_raw, stats, N, Sd, Sd, s, R.store8 ? 1 : 0);
    else
      np = launch_tail_join_fwd(dt(), s2, sc, params + tail.off, params + tail_bias, r_raw, stats, N, Sd, Sd, s);
  } else {
    // Conv2d(16 -> out_ch, k3 p1, bias): GEMM rows padded to 16 in LDS, epilogue stores the out_ch real rows as NCHW f32
    GatherArgs a;
    down_args(a, ConvGeom{16, 16, 3, 1, 1}, N, Sd, Sd, Sd, Sd);
    a.x = in.y; a.w = ps.packed(tail_pack_f); a.y = r_raw; a.bias = params + tail_bias; a.stats = stats; a.y_planes = cfg.out_ch;
    np = launch_gather_gemm(dt(), DT_F32, a, s);
  }
  MM_TRY(np);
  MM_TRY(bn_fwd(ps, bn_out, np, (double)N * Sd * Sd, s));
  MM_TRY(launch_affine_nchw(r_raw, ps.rows(bn_out).affine(), recon, N, cfg.out_ch, Sd * Sd, s));
  return MMVAE_OK;
}

int Net::decoder_bwd(int N, const float* d_recon, const float* params, float* grads, void* ws, size_t ws_bytes, float* d_enc,
                     hipStream_t s, const GaussTail* gauss) {
  Pass ps;
  MM_TRY(begin_pass(ps, N, ws, ws_bytes, params, grads));
  const Plan& P = *ps.P;
  char* const base = ps.base;
  float* const part = ps.part;
  float* r_raw = reinterpret_cast<float*>(base + P.r_raw);
  float* d_raw = reinterpret_cast<float*>(base + P.d_raw);
  const BnRows r0 = ps.rows(dbn0), ro = ps.rows(bn_out);
  const NetRoute& R = P.route;
  const int HW = Sd * Sd;
  pack_batch_begin();
  MM_TRY(packs_dec_bwd(ps, d_enc != nullptr, s));
  MM_TRY(pack_batch_flush(dt(), s));
  // the encoder stem's patch gram matrix (input only; stem_bwd.hip): here the side stream is idle for ~1 ms beside HBM-bound kernels, at the
  // start of encoder_bwd it ran beside the latency-bound kernels around the latent code and held their small launches up (lesson 55)
  if (R.stem_bwd_fused && !gram_ready_ && gram_fwd_N_ == N && gram_fwd_ws_ == ws && wgrad_stream(s) != s) {
    MM_TRY(side_fork(s));
    MM_TRY(launch_stem_gram(dt(), base + P.x_t, reinterpret_cast<float*>(base + P.stem_gram), 1024L * stem_bwd_part_floats(),
                            reinterpret_cast<double*>(base + P.stem_R), N, cfg.S, H1, W1, wgrad_stream(s)));
    if (hipEventRecord(gram_ev_, side_) != hipSuccess) { set_error("side stream mark failed"); return MMVAE_ERR_HIP; }
    gram_ready_ = true;
    // (the encoder backward's weight packs enqueued here as well -- 26 us off the caller's stream at the latent boundary -- change nothing:
    // 6.018 vs 6.018 ms over three A/B pairs; not kept)
  }
  // ---- output BN backward, tail conv backward
  int np = gauss ? launch_gauss_tail_reduce(r_raw, ro.affine(), gauss->target, gauss->sigma, gauss->coef, gauss->gscale, part, N, cfg.out_ch, HW, s)
                 : launch_bn_bwd_reduce_nchw(d_recon, r_raw, N, cfg.out_ch, HW, part, s);
  MM_TRY(np);
  // (the tail conv's bias gradient, sum of d_raw per output channel, in closed form from the same sums: BnBwdFinalizeArgs::dbias_conv)
  MM_TRY(bn_backward_coefs(ps, bn_out, np, 1, 0, (double)N * HW, s, grads + tail_bias));
  if (gauss)
    MM_TRY(launch_gauss_tail_apply(r_raw, ro.affine(), ro.coef(), gauss->target, gauss->sigma, gauss->coef, gauss->gscale, d_raw, N, cfg.out_ch,
                                   HW, s));
  else
    MM_TRY(launch_bn_bwd_apply_nchw(d_recon, r_raw, ro.coef(), d_raw, N, cfg.out_ch, HW, s));
  if (!R.tail_wg_in_reduce) {      // (else the forward did not store the joined activation: the join-backward reduce pass below recomputes it)
    // dW[oc][ci][kh][kw]: P = d_raw (planar f32, out_ch planes staged as 16 zero-padded channels), G = the last up-block's output
    WgradArgs a;
    wgrad_args(a, ConvGeom{16, 16, 3, 1, 1}, N, MapIn(d_raw, Sd, Sd), MapIn(base + dec.back().out, Sd, Sd), grads + tail.off, ps.wscratch);
    a.P_planar = 1; a.P_planes = cfg.out_ch; a.Ca_valid = cfg.out_ch;
    MM_TRY(side_fork(s));
    MM_TRY(launch_wgrad(dt(), a, wgrad_stream(s)));
  }
  int cur = 0;
  if (!R.tail_bwd_fused) {          // (else the last up-block's join backward recomputes the tail conv's input gradient from d_raw)
    // dx[n,h,w,ci] = sum dy[n,oc,h+1-kh,w+1-kw] * w[oc][ci][kh][kw]: planar f32 source padded to 8 channels in LDS
    GatherArgs a; std::memset(&a, 0, sizeof(a));
    a.x = d_raw; a.w = ps.packed(tail_pack_d); a.y = base + P.g[cur]; a.x_planar = 1; a.x_planes = cfg.out_ch;
    a.N = N; a.Hi = Sd; a.Wi = Sd; a.Cin = 8; a.Ho = Sd; a.Wo = Sd; a.Cout = 16; a.SI = 1; a.SO = 1;
    a.nphase = 1; a.phases[0] = Phase{0, 0, Sd, Sd, 9, 0, 0};
    for (int kh = 0; kh < 3; ++kh) for (int kw = 0; kw < 3; ++kw) a.taps[kh * 3 + kw] = Tap{1 - kh, 1 - kw};
    MM_TRY(launch_gather_gemm(dt(), dt(), a, s));
  }
  const int nd = (int)dec.size();
  for (int i = nd - 1; i >= 0; --i) {
    Block& B = dec[i];
    const bool jg = B.r.bwd_join_grad;     // join-gradient form: g[cur] is already masked by this block's join ReLU (the block above did it)
    const long npi = (long)N * B.Hin * B.Win;
    // the block input under its prologue: the stem's BatchNorm + ReLU for block 0 -- unless (blocks > 1) it has an identity shortcut and reads the
    // stem's materialised activation
    const BnSide in = i > 0 ? BnSide{base + dec[i - 1].out} : cfg.blocks > 1 ? BnSide{base + P.act0d} : BnSide{base + P.y0d, r0.affine()};
    const BnSide s1 = ps.rows(B.b1).side(base + B.y1), s2 = ps.rows(B.b2).side(base + B.y2), sc = ps.shortcut(B, in);
    const int ds = i & 1;          // dy set of this block (see encoder_bwd)
    const void *const dy1 = base + P.dy1[ds], *const dy2 = base + P.dy2[ds], *const dys = base + P.dys[ds];
    if (i + 2 <= nd - 1) MM_TRY(side_wait_mark(i + 2, s));
    const bool from_tail = R.tail_bwd_fused && i == nd - 1;
    // an identity shortcut's gradient is the masked incoming gradient itself: it goes straight into the block-input gradient
    const long dyso = B.identity ? P.g[cur ^ 1] : P.dys[ds];
    if (from_tail) {
      np = launch_tail_join_bwd_reduce(dt(), d_raw, params + tail.off, s2, sc, part, cfg.out_ch, N, Sd, Sd, s,
                                       R.tail_wg_in_reduce ? ps.wscratch : nullptr, R.store8 ? 1 : 0);
      MM_TRY(np);
      if (R.tail_wg_in_reduce) {
        MM_TRY(side_fork(s));
        MM_TRY(launch_tail_wgrad_finalize(ps.wscratch, np, grads + tail.off, wgrad_stream(s)));
      }
      MM_TRY(join_backward(ps, B, sc, nullptr, false, nullptr, nullptr, s, np));       // (the sums are there: the coefficients only)
    } else   // (join-gradient form: no apply pass, the two fused passes below evaluate dy2 / dys from g[cur], y2 / ys and the coefficients)
      MM_TRY(join_backward(ps, B, sc, base + P.g[cur], jg, jg ? nullptr : base + P.dy2[ds], base + dyso, s));
    if (B.r.bwd_join_stream) {   // the whole block in one pass (conv_joinbwd.hip); conv1 (1x1) follows once bn1's sums are final
      float* ws2 = reinterpret_cast<float*>(base + P.wscratch2);
      JoinBwdLaunch L;
      L.d_raw = d_raw; L.w_tail = params + tail.off; L.y2 = s2; L.ys = sc;
      L.y1 = s1; L.wd2 = ps.packed(B.c2.packD); L.da1 = base + P.da1; L.part2 = ws2; L.bn_part = part;
      L.xin = in; L.wds = ps.packed(B.cs.packD); L.gin = base + P.g[cur ^ 1];
      L.parts = ws2 + 1024L * 4096;                        // (at most 1024 blocks, one [16][16][16] partial image per conv each)
      L.N = N; L.f8in = R.store8 ? 1 : 0;
      const int nb = launch_join_bwd_stream(L, s);
      MM_TRY(nb);
      MM_TRY(reduce_wgrad_parts(ps, B.c2, L.part2, nb, 16, s));
      MM_TRY(reduce_wgrad_parts(ps, B.cs, L.parts, nb, 16, s));
      MM_TRY(bn_backward_coefs(ps, B.b1, nb, 1, 0, (double)npi, s));
      Conv1BwdLaunch C1;
      C1.da1 = base + P.da1; C1.y1 = s1; C1.xin = in; C1.w1u = ps.packed(B.c1.packU);
      C1.gin = base + P.g[cur ^ 1]; C1.part = ws2; C1.nrows = (long)N * B.Hin;
      C1.mask_out = (i > 0 && dec[i - 1].r.bwd_join_grad) ? 1 : 0;
      const int nb1 = launch_conv1_bwd_stream(C1, s);
      MM_TRY(nb1);
      MM_TRY(reduce_wgrad_parts(ps, B.c1, ws2, nb1, 1, s));   // conv1: Conv2d weight (out = 16, in = Cin): partial images [out][in]
      MM_TRY(side_mark(i));
      cur ^= 1;
      continue;
    }
    if (from_tail)
      MM_TRY(launch_tail_join_bwd_apply(dt(), d_raw, params + tail.off, s2, sc, base + P.dy2[ds], base + P.dys[ds], cfg.out_ch, N, Sd, Sd, s));
    hipStream_t wsm = wgrad_stream(s);
    MM_TRY(side_fork(s));
    const bool fuse_c2 = B.r.bwd_fuse_c2, fuse_cs = B.r.bwd_fuse_cs;
    int np_b1 = 0;                       // rows of bn1's backward sums when the fused pass has left them in `part`
    if (B.identity) {
      // conv2 (3x3 Conv2d): wgrad(P = dy2, G = a1 with BN+ReLU prologue); dgrad -> d_a1
      MM_TRY(run_wgrad(ps, B.c2, BnSide{dy2}, s1, wsm));
      MM_TRY(run_up(ps, B.c2, dy2, base + P.da1, s));
    } else {
      // conv2 (ConvT k4 s2): wgrad(P = a1 small side with BN+ReLU prologue, G = dy2 large side); dgrad = strided conv -> d_a1; fused: ONE pass over dy
      if (!fuse_c2) MM_TRY(run_wgrad(ps, B.c2, s1, BnSide{dy2}, wsm));
      if (!fuse_cs) MM_TRY(run_wgrad(ps, B.cs, in, BnSide{dys}, wsm));
      if (fuse_c2) {
        // ... and bn1's backward sums come out of the same pass (the data gradient is in registers, y1 is the pass's P operand)
        WgradOpts o;
        o.scratch = reinterpret_cast<float*>(base + P.wscratch2); o.scale = B.c2.wscale; o.bn_part = B.C == 16 ? part : nullptr; o.jg = jg ? &s2 : nullptr;
        const int rcf = op_run_bwd_fused(dt(), geom(B.c2), ps.packed(B.c2.packD), MapIn(s1, B.Hin, B.Win), MapIn(jg ? base + P.g[cur] : dy2, B.Hout, B.Wout),
                                         SecondSrc(), base + P.da1, grads + B.c2.off, N, s, o);
        if (rcf <= 0) { if (rcf == 0) set_error("decoder_bwd: fused backward of %s not taken", "conv2"); return rcf < 0 ? rcf : MMVAE_ERR_UNSUPPORTED; }
        if (B.C == 16) np_b1 = rcf;
      } else
        MM_TRY(run_down(ps, B.c2, dy2, base + P.da1, s));
    }
    MM_TRY(bn_relu_backward(ps, B.b1, base + P.da1, s1.y, base + P.dy1[ds], npi, s, np_b1));
    // conv1 (1x1): wgrad(P = dy1, G = xin); upsample (ConvT): wgrad(P = xin, G = dys)
    MM_TRY(side_fork(s));
    // (with the fused shortcut pass below the 1x1 conv's weight gradient comes out of that pass: dy1 and the block input are its rows)
    if (!fuse_cs) MM_TRY(run_wgrad(ps, B.c1, BnSide{dy1}, in, wsm));
    MM_TRY(side_mark(i));
    if (B.identity)     // d_xin already holds the shortcut's share: the 1x1 conv's data gradient is added to it
      MM_TRY(run_up(ps, B.c1, dy1, MapOut::add(base + P.g[cur ^ 1]), s));
    else if (fuse_cs) {  // shortcut ConvT: weight gradient + data gradient + the 1x1 conv's share (dy1 (x) w1) and ITS weight gradient, one pass over dys
      SecondSrc x2;
      x2.x2 = dy1; x2.w2 = ps.packed(B.c1.packU);
      WgradOpts o;
      o.scratch = reinterpret_cast<float*>(base + P.wscratch2); o.scale = B.cs.wscale; o.dW2 = grads + B.c1.off; o.scale2 = B.c1.wscale; o.jg = jg ? &sc : nullptr;
      const int rcf = op_run_bwd_fused(dt(), geom(B.cs), ps.packed(B.cs.packD), MapIn(in, B.Hin, B.Win), MapIn(jg ? base + P.g[cur] : dys, B.Hout, B.Wout),
                                       x2, base + P.g[cur ^ 1], grads + B.cs.off, N, s, o);
      if (rcf <= 0) { if (rcf == 0) set_error("decoder_bwd: fused backward of %s not taken", "upsample"); return rcf < 0 ? rcf : MMVAE_ERR_UNSUPPORTED; }
    } else              // one kernel: the 1x1 conv's data gradient (dy1, already on this block's input grid) is a second source of the shortcut's
      MM_TRY(run_down(ps, B.cs, dys, base + P.g[cur ^ 1], s, &B.c1, dy1));
    cur ^= 1;
  }
  // ---- decoder stem
  if (dec.size() >= 2) MM_TRY(side_wait_mark(1, s));   // the stem uses dy set 1 (block index -1)
  MM_TRY(bn_relu_backward(ps, dbn0, base + P.g[cur], base + P.y0d, base + P.dy1[1], (long)N * 4, s));
  MM_TRY(side_fork(s));
  const void* const dy0 = base + P.dy1[1];
  MM_TRY(run_wgrad(ps, dstem, BnSide{base + P.enc_t}, BnSide{dy0}, wgrad_stream(s)));
  if (d_enc) {
    MM_TRY(run_down(ps, dstem, dy0, base + P.dh, s));
    MM_TRY(launch_convert(dt(), DT_F32, base + P.dh, d_enc, (long)N * cfg.z, s));
  }
  if (!defer_join_) MM_TRY(side_join(s));
  return MMVAE_OK;
}

}  // namespace mmvae
