// Host-side launch API of the HIP kernels (internal; the public C ABI is include/mmvae.h).
#pragma once
#include "common.hpp"

namespace mmvae {

enum DType : int { DT_F32 = 0, DT_BF16 = 1 };
inline size_t dtype_size(int dt) { return dt == DT_F32 ? 4 : 2; }

// ---------------------------------------------------------------- a tensor seen through its BatchNorm
// The launchers below take each such tensor as ONE argument: sides of a join first, then outputs, then the shape, then the stream.
struct Affine { const float* scale = nullptr; const float* shift = nullptr; };                      // folded forward BatchNorm; both null: the tensor as it is
struct BnCoef { const float* A = nullptr; const float* B = nullptr; const float* C = nullptr; };   // backward: dy = A*g + B*y + C (bn_bwd_finalize)
// a pre-BatchNorm tensor with its rows: one side of a residual join, or a consumer's input under its BatchNorm + ReLU prologue (bwd unused)
struct BnSide { const void* y = nullptr; Affine fwd; BnCoef bwd; };

// ---------------------------------------------------------------- the conv path's operands (conv_ops.hpp, the stream launchers below, Net::run_*)
// One argument per tensor here as well, in the same order: input maps, output maps, the batch size, the stream, then defaulted options.
// An input map: the tensor [N][H][W][C], and the prologue its consumer applies on load, relu?(x * pro.scale + pro.shift) (pro empty: x as it is).
// From a BnSide the ReLU is on: a consumer's input under its BatchNorm + ReLU.  Without a size (Net::run_*) the callee fills it in from the layer.
struct MapIn {
  const void* x = nullptr; int H = 0, W = 0; Affine pro; int relu = 0;
  MapIn() = default;
  MapIn(const void* x_) : x(x_) {}
  MapIn(const void* x_, int H_, int W_, Affine pro_ = Affine(), int relu_ = 0) : x(x_), H(H_), W(W_), pro(pro_), relu(relu_) {}
  MapIn(const BnSide& t) : x(t.y), pro(t.fwd), relu(1) {}
  MapIn(const BnSide& t, int H_, int W_, int relu_ = 1) : x(t.y), H(H_), W(W_), pro(t.fwd), relu(relu_) {}
  // the operand of a shape query: no data; has_pro says whether the launch will carry a prologue -- the predicates test pro.scale for null and
  // read nothing through it, so it points at a constant here and nowhere else
  static MapIn shape(int H_, int W_, bool has_pro = false) {
    static const float one = 1.f;
    return has_pro ? MapIn(nullptr, H_, W_, Affine{&one, &one}, 1) : MapIn(nullptr, H_, W_);
  }
};
// An output map: the tensor, the BatchNorm statistics rows its producer leaves (nullable), and whether the result is added to what y holds.
struct MapOut {
  void* y = nullptr; int H = 0, W = 0; float* stats = nullptr; int accumulate = 0;
  MapOut() = default;
  MapOut(void* y_, float* stats_ = nullptr) : y(y_), stats(stats_) {}
  MapOut(void* y_, int H_, int W_, float* stats_ = nullptr, int accumulate_ = 0) : y(y_), H(H_), W(W_), stats(stats_), accumulate(accumulate_) {}
  static MapOut add(void* y_, int H_ = 0, int W_ = 0) { return MapOut(y_, H_, W_, nullptr, 1); }     // y += result
};

// ---------------------------------------------------------------- gather GEMM
// y[n, hq*SO+ph, wq*SO+pw, co] (+)= bias[co] + sum_{t<ntaps} sum_{ci}
//        pro(x[n, hq*SI+dh[t], wq*SI+dw[t], ci]) * w[co][t][ci]
// with zero for out-of-range input coordinates (zero padding is applied AFTER pro()).
// Covers Conv2d forward (SI=stride, SO=1, one launch) and every stride-phase of a
// transposed convolution / data-gradient (SI=1, SO=stride, one launch per phase).
struct Tap { int dh, dw; };
constexpr int kMaxTaps = 25;     // over all phases of one launch (5x5 stem)
constexpr int kMaxPhases = 4;
struct Phase { int ph, pw, Hq, Wq, ntaps, tap0; long w_off; /* element offset of this phase's [Cout][ntaps*Cin] matrix */ };
struct GatherArgs {
  const void* x; const void* w; void* y;
  const float* pro_scale; const float* pro_shift; int pro_relu;
  const float* bias;
  float* stats;            // [gridDim.z*gridDim.x][2][Cout] partial (sum, sumsq) of the f32 results, or null
  int accumulate;          // y += result
  int N, Hi, Wi, Cin, Ho, Wo, Cout;
  int SI, SO;
  int nphase; Phase phases[kMaxPhases]; Tap taps[kMaxTaps];
  int cin_vecs;
  // optional boundary layouts (patch-tile kernels only):
  int x_planar, x_planes;  // 1: x is planar f32 [N][x_planes][Hi][Wi], 2: planar T; staged as Cin=16 channels, zero padded
  int y_planes;            // >0: y is NCHW f32 [N][y_planes][Ho][Wo] (Cout = 16 padded GEMM rows; stats rows have y_planes channels)
  // optional SECOND source (patch-tile kernel only; launch_gather_gemm returns MMVAE_ERR_UNSUPPORTED when it cannot take it):
  // y[q-pixel of phase (x2_ph, x2_pw)] += sum_c2 x2[n, hq, wq, c2] * w2[co][c2] -- a 1x1 convolution of a tensor that lives on the
  // q grid itself ([N][Hq][Wq][Cin2] of T, no halo).  Merges the two data gradients that meet at a residual block's input
  // (3x3 / 4x4 main path + 1x1 shortcut) into one kernel: no read-modify-write of the sum.
  const void* x2; const void* w2; int Cin2, x2_ph, x2_pw;
  int fp8;                 // 1: w holds e4m3 bytes (same [cout][tap][cin] order); only the deep-layer kernel takes it (else an error)
  int wfrag, wfrag2;       // 1: w (w2) is packed fragment-major (PackArgs::frag); only deep2_conv_kernel / pos_conv_kernel read it (else an error)
  int gk, gs, gp, gup;     // the conv-like weight's (k, s, p) and the form (1: down, 2: up) when the launch comes from op_run_down / op_run_up (0: unknown)
};
// out_dt: dtype of y (may be DT_F32 while x/w are bf16).  Returns the number of stats partial rows (>0) or an error (<0).
int launch_gather_gemm(int dt, int out_dt, GatherArgs a, hipStream_t s);
// Whether deep2_conv_kernel (conv_deep2.inc; a.fp8: its e4m3 form) / pos_conv_kernel (conv_pos.inc) takes the launch when the dispatcher offers
// it: the dispatcher's own code, stopped in front of the launch.  These two read fragment-major weights (a.wfrag), so whoever packs a layer asks
// here.  The data pointers of `a` are not looked at (they may be null), except that a.x2 / a.bias / a.pro_scale say whether there is one.
bool gather_deep2_takes(int dt, int out_dt, const GatherArgs& a);
bool gather_pos_takes(int dt, int out_dt, const GatherArgs& a);
constexpr int kGatherMaxGridX = 1024;

// ---------------------------------------------------------------- wgrad
// dW[a*sA + b*sB + tap_off[t]] += scale * sum_{n,hp,wp} proP(P[n,hp,wp,a]) * proG(G[n, hp*stride-pad+kh_t, wp*stride-pad+kw_t, b])
struct WgradArgs {
  const void* P; const void* G; float* dW;
  const float* proP_scale; const float* proP_shift; int proP_relu;
  const float* proG_scale; const float* proG_shift; int proG_relu;
  int N, Hp, Wp, Ca, Hg, Wg, Cb;
  int Cb_valid;            // b >= Cb_valid is computed but not written (0 -> Cb)
  int Ca_valid;            // likewise for a (0 -> Ca)
  int P_planar, P_planes;  // 1: P is planar f32 [N][P_planes][Hp][Wp] (patch-tile kernel only; Ca = 16, Ca_valid = P_planes)
  float* scratch;          // optional, kWgradScratchBytes: per-block partial images [part][tap][a][b], summed by wgrad_reduce_kernel
  int stride, pad, ksz;
  int sA, sB; int ntaps; int tap_off[25];
  float scale;
  int M, pix_per_block;
  int TA16, TB16, TG;      // tile config chosen by the launcher
  struct WgradReduceArgs* defer;   // optional (stream kernels only): the reduce is NOT launched, its arguments are left here (nparts = 0 when the
                                   // launch took another kernel and reduced at once) -- the caller launches it later, off the busy phase
};
int launch_wgrad(int dt, WgradArgs a, hipStream_t s);
int try_wgrad_pos(int dt, const WgradArgs& a, hipStream_t s);     // conv_wpos.hip: both maps 1x1 .. 4x4 (1 = taken, 0 = not this kernel's shape)
bool wgrad_stream_shape(int dt, const WgradArgs& a);
int try_wgrad_stream(int dt, const WgradArgs& a, hipStream_t s);   // conv_wstream.hip: 1 = taken, 0 = not this kernel's shape, <0 error
int try_wgrad_stream_pair(int dt, const WgradArgs& a, const void* P2, float* dW2, float scale2, hipStream_t s);
// weight gradient + data gradient (w.r.t. P) of a 16 -> 16 channel k4 s2 layer in one pass over G (conv_wstream.hip)
bool dgrad_wgrad_stream_shape(int dt, const WgradArgs& a);
// dW2 (optional, with x2): the 1x1 conv's own weight gradient [16][Ca] += scale2 * x2^T (x) pro(P), from the same pass
// jg: dy of a BatchNorm behind a residual join, evaluated by the consumer's loader: dy = A[c] * g + B[c] * y + C[c] (jg->bwd), g = the join's
// output gradient already masked by its ReLU, y = the branch's pre-BatchNorm output (conv_wstream.hip, JG)
bool dgrad_wgrad_stream_jg_shape(int dt, const WgradArgs& a, bool has_x2, bool bn_sums);
int try_dgrad_wgrad_stream(int dt, const WgradArgs& a, const void* wd, void* dx, const void* x2, const void* w2, float* bn_part, hipStream_t s,
                           float* dW2 = nullptr, float scale2 = 1.f, const BnSide* jg = nullptr);

// ---- last up-block backward in one pass (conv_joinbwd.hip): the join's BatchNorm backward (incoming gradient recomputed from the
// one-plane reconstruction gradient), both ConvTranspose2d weight gradients and data gradients, bn1's backward sums -- dy2 / dys are
// never stored.  bf16, 16 channels, 32x32 -> 64x64, one output plane.
struct JoinBwdLaunch {
  const float* d_raw; const float* w_tail;
  BnSide y2, ys;           // the two branch outputs at the join, under bn2 / the shortcut's BatchNorm
  BnSide y1; const void* wd2; void* da1; float* part2; float* bn_part;   // main path (conv2): its input under bn1 + ReLU (fwd required)
  BnSide xin; const void* wds; void* gin; float* parts;                  // shortcut (upsample): the block input under its prologue, if any
  int N;
  int f8in = 0;            // y2 / ys are e4m3 bytes (16 per pixel): fp8 mode's storage of these two tensors
};
bool join_bwd_stream_ok(int dt, int OC, int C, int Hp, int Hg);
int launch_join_bwd_stream(const JoinBwdLaunch& L, hipStream_t s);    // returns blocks = partial images per conv = rows of bn_part
// ... and the block's 1x1 conv afterwards: dy1 from d_a1 (bn1 backward), g_in += dy1 (x) W1 in place, dW1 partial images [blocks][16][16]
struct Conv1BwdLaunch {
  const void* da1; BnSide y1;      // conv1's output under bn1: ReLU mask from fwd, dy1 from bwd
  BnSide xin; const void* w1u; void* gin; float* part; long nrows;
  int mask_out = 0;   // g_in leaves masked by the ReLU that produced xin (xin > 0): the block below evaluates its BatchNorm backward on load (jg)
};
int launch_conv1_bwd_stream(const Conv1BwdLaunch& L, hipStream_t s);  // returns blocks
// conv_joinfwd.hip: a block's residual join fused with the next block's 1x1 conv1 (16 outputs) and bn1's statistics; C = joined channels (16 / 32)
bool join_conv1_fwd_ok(int dt, int C, int Cout_next, long npix);
int launch_join_conv1_fwd(const BnSide& y2, const BnSide& ys, const void* w1_down, void* out, void* y1, float* stats, int C, long npix,
                          hipStream_t s);   // returns the rows of `stats`

// ---------------------------------------------------------------- v2 patch-tile kernels (conv_tile.hip)
// A tile is up to TP (128, or 64/32 for wgrad on tiny feature maps) q-pixels: `qr` consecutive q-rows of one image (tiles_per_img > 0) or `segs` whole images.
// Its input patch per segment is PR x PW pixels starting at input (hq0*SI + oh, ow).
// A tile may hold `sub` (1,2,4) consecutive 128-pixel sub-tiles staged behind ONE barrier pair: sub-tile s starts `sub_j`*s
// q-rows (or `sub_seg`*s images) further, i.e. `sub_pix`*s patch pixels further.
struct TileGeom { int N, Hq, Wq, Hi, Wi, SI, oh, ow, segs, qr, PR, PW, tiles_per_img, ntiles, TP, sub, sub_j, sub_seg, sub_pix; };
bool make_tile_geom(TileGeom& g, int N, int Hq, int Wq, int Hi, int Wi, int SI, int oh, int ow, int span_h, int span_w, int TP = 128,
                    int sub = 1);
struct Wgrad2Args {
  const void* P; const void* G; float* dW;   // dW: the partial-image scratch [gridDim.x][ntaps][Ca][Cb] (plain stores)
  const float* proP_scale; const float* proP_shift; int proP_relu;
  const float* proG_scale; const float* proG_shift; int proG_relu;
  TileGeom g;
  int Ca, Cb, Cb_valid, Ca_valid, ksz, ntaps, TG;
  int sA, sB; int tap_off[25]; float scale;
  int P_planar, P_planes;  // 1: P is planar f32 [N][P_planes][Hq][Wq] staged as Ca = 16 zero-padded channels
  int nw;                  // waves per block: 4, or 9 / 16 = one tap per wave (deep 3x3 / 4x4 layers)
  // 1 (what the launcher sets): tap-split blocks store their accumulators straight into the partial image; 0: through the LDS image of the
  // k-split flush (same result).  Kept as a runtime value: with the test resolved at compile time the 16x16-tile instantiations spill
  // (0 -> 32..196 bytes of scratch)
  int partial;
};
size_t wgrad2_lds_bytes(const Wgrad2Args& a, int dt, int TA, int TB);
int wgrad2_patch_slots(const Wgrad2Args& a, int dt, int TB);
int wgrad2_taps_per_block(int ta16, int tb16, int ntaps);
int launch_wgrad2(int dt, const Wgrad2Args& a, int gx, int tiles_ab, int zg, int ta16, int tb16, hipStream_t s);
size_t gather3_lds_bytes(const GatherArgs& a, int dt, int CT);
int launch_gather3(int dt, int out_dt, const GatherArgs& a, int gx, hipStream_t s);
struct WgradReduceArgs { const float* part; float* dW; int Ca, Cb, ntaps, nparts, Ca_valid, Cb_valid, sA, sB; int tap_off[25]; float scale; int exclusive;
                         long part_stride; /* floats between two partial images (0: ntaps * Ca * Cb) */ };
// the reduce of the nparts partial images a kernel left at `part` for the weight gradient `a`: a's image shape, weight strides, taps and scale
inline WgradReduceArgs reduce_args(const WgradArgs& a, const float* part, int nparts) {
  WgradReduceArgs u = {};
  u.part = part; u.dW = a.dW; u.Ca = a.Ca; u.Cb = a.Cb; u.ntaps = a.ntaps; u.nparts = nparts;
  u.Ca_valid = a.Ca_valid; u.Cb_valid = a.Cb_valid; u.sA = a.sA; u.sB = a.sB; u.scale = a.scale;
  for (int t = 0; t < 25; ++t) u.tap_off[t] = a.tap_off[t];
  return u;
}
// ... and of whole images [Ca][Cb][ntaps] into a dense weight of that shape (the fused backward passes' partial images)
inline WgradReduceArgs reduce_args(const float* part, int nparts, float* dW, int Ca, int Cb, int ntaps, float scale = 1.f) {
  WgradReduceArgs u = {};
  u.part = part; u.dW = dW; u.Ca = Ca; u.Cb = Cb; u.ntaps = ntaps; u.nparts = nparts;
  u.Ca_valid = Ca; u.Cb_valid = Cb; u.sA = Cb * ntaps; u.sB = ntaps; u.scale = scale;
  for (int t = 0; t < ntaps && t < 25; ++t) u.tap_off[t] = t;
  return u;
}
int launch_wgrad_reduce(WgradReduceArgs a, hipStream_t s);
int wgrad_reduce_check(WgradReduceArgs a);        // launch_wgrad_reduce's refusals alone (< 0), nothing enqueued: asked before the producing kernel is
constexpr size_t kWgradScratchBytes = 64u << 20;   // capacity of the partial-image scratch every wgrad caller provides
// ---- pipelined all-phases patch kernel (conv_patch.hip)
struct PatchPhase { int ph, pw, Hq, Wq, ntaps, tap0; long w_off; int w_vec0, koff0; };
struct PatchArgs {
  const void* x; const void* w; void* y;
  const float* pro_scale; const float* pro_shift; int pro_relu;
  const float* bias; float* stats; int accumulate;
  int Cin, Cout, Ho, Wo, SO;
  TileGeom g;                  // one geometry for all phases: q-grid = max over phases, patch = union of the tap spans
  int nphase; PatchPhase phases[kMaxPhases]; Tap taps[kMaxTaps];
  int w_vecs, koff_total;      // LDS carve: weight vec16s of all phases, k-offset ints of all phases
  int x_planar, x_planes, y_planes;
  int npt, wq_shift;           // 16-pixel column tiles per wave (2, 4, 8); log2(Wq) when npt > 2
  int uni, out_wave_bytes;     // uniform geometry: LDS-staged epilogue, bytes of one wave's staging buffer
  int phase_of[4];             // uni: phase index of output sub-position (ph, pw) = [ph*SO + pw]
  unsigned x_bytes;            // size of x in bytes (< 2^31): buffer-load range for the NHWC staging
  // second source (see GatherArgs): [N][Hq][Wq][Cin2] on the q grid, weights [Cout][Cin2], added into phase x2_phase
  const void* x2; const void* w2; int Cin2, x2_phase, kvp2, w2_vec0, x2_vec0, x2_slots; unsigned x2_bytes;
};
size_t patch_conv_lds_bytes(const PatchArgs& a, int dt);
void patch_conv_x2_carve(PatchArgs& a, int dt);
int patch_conv_slots(const PatchArgs& a, int dt);
int launch_patch_conv(int dt, int out_dt, const PatchArgs& a, int gx, hipStream_t s);   // returns stats rows (= gx) or <0
// ---- deep-layer implicit GEMM (conv_deep2.inc): resident unpadded patch, weights from L2 straight into MFMA fragments
using DeepPhase = Phase;
struct DeepArgs {
  const void* x; const void* w; void* y;
  const float* pro_scale; const float* pro_shift; int pro_relu;
  const float* bias; float* stats; int accumulate;
  int N, Hi, Wi, Cin, Ho, Wo, Cout, SI, SO;
  int Hq, Wq;                  // q-grid of a tile image (max over phases)
  int nphase; DeepPhase phases[kMaxPhases]; Tap taps[kMaxTaps]; int ntaps_all;
  int ipt, ntiles;             // whole images per tile, tiles
  int ct16, npt;               // cout tile / 16 (4 or 8), 16-pixel column tiles per wave
  int fp8;                     // w is e4m3 bytes, activations are quantised in LDS: v_mfma_f32_16x16x32_fp8_fp8 (forward convs, bf16 storage)
  int nw, cpt_log2;            // deep2_conv_kernel: waves per block (32 couts each), log2(64-byte chunks per tap of a weight row)
  int wfrag;                   // weights are fragment-major (PackArgs::frag)
};
size_t deep2_conv_lds_bytes(const DeepArgs& a, int dt);
int launch_deep2_conv(int dt, int out_dt, const DeepArgs& a, int gx, hipStream_t s);  // conv_deep2.inc; returns stats rows (= gx) or <0
// ---- position-major implicit GEMM for q-grids up to 4x4 (conv_pos.inc; bf16, fragment-major weights): an MFMA column is an image, so
// (position, tap) pairs that fall into the zero padding are not computed at all
struct PosArgs {
  const void* x; const void* w; void* y;
  const float* pro_scale; const float* pro_shift; int pro_relu;
  float* stats; int accumulate;
  int N, Cout;
  int nw;                      // waves per block (32 couts each); grid.y = Cout / (32 nw)
  int ntiles;                  // set by the launcher
};
// up = 0: "down" form (Conv2d forward / ConvT data gradient), up = 1: "up" form; HI / HO input / output map size.  Returns stats rows (> 0),
// 0 when no instantiation takes the geometry, < 0 on error.  a == nullptr: nothing is launched, 1 when an instantiation takes the geometry.
int launch_pos_conv(int K, int S, int P, int up, int HI, int HO, int CIN, const PosArgs* a, hipStream_t s);

// ---------------------------------------------------------------- weight packing
// dst[(col*ntaps + t)*K + k] = T(scale * src[col*s_col + k*s_k + tap_off[t]])
struct PackArgs {
  const float* src; void* dst; int cols, K, ntaps; int s_col, s_k; int tap_off[kMaxTaps]; float scale;
  int cols_valid, K_valid;   // >0: columns / k beyond these are written as zero (channel padding), source not read
  int fp8;                   // 1: dst receives OCP e4m3 bytes (one per element) instead of T
  // 1: fragment-major order for deep2_conv_kernel: the [cols][ntaps*K] matrix is cut into 16-column x 64-byte blocks, each stored as the
  // 1 KB one wave loads as an MFMA A fragment (lane = 16*g + r holds 16 bytes: column 16*blk + r, bytes 16*g .. of the block's chunk):
  // dst[((blk * nchunks + chunk) * 64 + 16*g + r) * VE + e]
  int frag;
};
int launch_pack(int dt, const PackArgs& a, hipStream_t s);
// Batched packing: between pack_batch_begin() and pack_batch_flush() every launch_pack() call is only recorded;
// flush packs all recorded jobs with ONE kernel (grid.y = job).  Not re-entrant (one host thread per net).
void pack_batch_begin();
int pack_batch_flush(int dt, hipStream_t s);

// ---------------------------------------------------------------- stem im2col
// im2col of the 1-channel image for the stem weight gradient: col[m][32] (25 taps, 7 zero pads), T
int launch_stem_im2col(int dt, const void* x, void* col, int N, int H, int W, int Ho, int Wo, hipStream_t s);

// stem backward in one pass (stem_bwd.hip): BatchNorm sums + the three pixel reductions dW is an affine function of
bool stem_bwd_fusable(int S);
// 32 -> 32 channel 3x3 forward convs on 16-pixel-wide output maps as a per-wave stream, optionally with the block's 1x1 stride-2 shortcut
// from the same input rows (conv_fstream.hip): returns stats rows (> 0) or an error
bool conv3_stream_ok(int dt, int Cin, int Cout, int k, int s, int p, int Hin, int Win);
// dy (H x H, no prologue) -> dx, with the backward sums (dx.stats) of the BatchNorm + ReLU `mask` = the conv's input under its rows
int launch_conv3_stream_bwd(int dt, const MapIn& dy, const void* w_flipped, const BnSide& mask, const MapOut& dx, int N, hipStream_t s);
// x -> y (y.H x 16; x is stride * y.H wide), and (ysc.y, with wsc) the 1x1 stride-2 shortcut's output from the same rows
int launch_conv3_stream(int dt, int stride, const MapIn& x, const void* w, const void* wsc, const MapOut& y, const MapOut& ysc, int N,
                        hipStream_t s);
// ConvTranspose2d(16 -> 16, k4 s2 p1) forward on 16x16 / 32x32 inputs as a per-wave stream (conv_fstream.hip)
bool convT4_stream_ok(int dt, int Cin, int Cout, int k, int s, int p, int Hin, int Win);
int launch_convT4_stream(int dt, const MapIn& x, const void* w_up, const MapOut& y, int N, hipStream_t s, int f8out = 0);
// x.H x x.H -> twice that; f8out: y leaves as e4m3 bytes (32x32 inputs only); y.y == nullptr (not with f8out): the statistics alone, same partial rows
// last up-block join + one-plane tail conv as a per-wave MFMA stream (conv_fstream.hip; bf16, 64x64): returns stats rows or an error
bool tail_fwd_stream_ok(int dt, int OC, int H, int W);
int launch_tail_fwd_stream(int dt, const BnSide& y2, const BnSide& ys, const float* w, const float* bias, float* r_raw, float* stats, int N, int H,
                           int W, hipStream_t s, int f8in = 0);
// the same with the two branch outputs recomputed from the ConvTranspose2d inputs instead of read (conv_fstream.hip; bf16, 32x32 -> 64x64, 16 channels);
// y2 / ys (both or neither): the kernel also stores the branch outputs [N][64][64][16] bf16, bit-identical to launch_convT4_stream's
bool up5_tail_fwd_ok(int dt, int OC, int C, int Cin, int Hin, int Hout);
// y1 / xin: the two ConvTranspose2d inputs under their prologues (xin's may be empty); bn2 / bns: the folded BatchNorms of the recomputed branches
int launch_up5_tail_fwd(const BnSide& y1, const void* w2_up, const BnSide& xin, const void* wu_up, Affine bn2, Affine bns, const float* w,
                        const float* bias, float* r_raw, float* stats, int N, hipStream_t s, void* y2 = nullptr, void* ys = nullptr);
// stem forward as a per-wave stream (bf16; stem_bwd.hip): returns stats rows (> 0) or an error
bool stem_fwd_stream_ok(int dt, int S);
int launch_stem_fwd_stream(int dt, const void* x, const float* w, void* y, float* stats, int N, int S, hipStream_t s);
int stem_bwd_part_floats();
int launch_stem_gram(int dt, const void* x, float* scratch, long scratch_cap_floats, double* R, int N, int S, int Ho, int Wo, hipStream_t s);
int launch_stem_bwd(int dt, const void* g, const void* y0, const void* x, const float* ms, const float* mb, float* partials,
                    long partials_cap_floats, int N, int S, int Ho, int Wo, hipStream_t s);   // returns rows
bool stem_bwd_dg_ok(int dt, int S);
int launch_stem_bwd_dg(const void* dy1, const void* dys, const void* wd1, const void* wds, const void* y0, const void* x, const float* ms, const float* mb,
                       float* partials, long partials_cap_floats, int N, int S, int Ho, int Wo, hipStream_t s);   // returns rows
int launch_stem_bwd_finalize(const float* partials, int nparts, const double* R, const float* w, const float* global_sums, double count,
                             const float* gamma, const float* mean, const float* istd, float* dgamma, float* dbeta, float* dW, hipStream_t s);

// ---------------------------------------------------------------- BatchNorm pieces
// per-channel (sum, sumsq) partials over an NHWC tensor of T: out [nparts][2][C]; returns nparts
int launch_chan_stats_nhwc(int dt, const void* y, long npix, int C, float* partials, hipStream_t s);
int chan_stats_parts(long npix, int C);
// same for an NCHW f32 tensor [N][C][HW]
// training finalize: partials -> mean/istd/scale/shift; running stats update (momentum, unbiased var); nbt += 1
struct BnFinalizeArgs {
  float in_scale = 1.f;      // the statistics are of y' = in_scale * y (fp8 layers: statically scaled weights): eps and the running
                             // statistics are converted, so the BatchNorm of y' is exactly the BatchNorm of y
  const float* partials; int nparts; int C; double count;
  const float* gamma; const float* beta; float* running_mean; float* running_var; long long* nbt;
  float* mean; float* istd; float* scale; float* shift; float momentum, eps;
};
int launch_bn_finalize(const BnFinalizeArgs& a, hipStream_t s);
int launch_partial_rowsum(const float* partials, int nparts, int width, float* out, hipStream_t s, int row_stride = 0);   // SyncBN: [nparts][width (stride row_stride)] -> [width]
// eval: scale = gamma/sqrt(rv+eps), shift = beta - rm*scale
struct BnFoldEntry { int g_off, b_off, rm_off, rv_off, scale_off, shift_off, C; float in_scale; };
constexpr int kBnFoldMax = 96;                       // 96 x 32 B of kernel arguments per launch
struct BnFoldTable { BnFoldEntry e[kBnFoldMax]; };
int launch_bn_fold_eval(const BnFoldEntry* entries, int n, const float* params, const float* bnbuf, float* bnws, float eps, hipStream_t s);
// out = relu(bn(a.y) + bn(b.y)), bn = the side's fwd   (NHWC, T)
int launch_join_fwd(int dt, const BnSide& a, const BnSide& b, void* out, long npix, int C, hipStream_t s);
// out = relu?(bn(a.y))
int launch_affine_act(int dt, const BnSide& a, int relu, void* out, long npix, int C, hipStream_t s);
// BN-backward reductions over side a (and side b when b.y != null: a residual join).  g = dout * mask, mask = (out > 0) if out != null, else
// (bn(a.y) > 0) if a.fwd.scale, else 1; a join with b.fwd.scale as well masks by bn(a.y) + bn(b.y) > 0 (the join recomputed, `out` not read).
// partials [nparts][1+NY][C]: sum g, sum g*a.y, (sum g*b.y).  Returns nparts.
int launch_bn_bwd_reduce(int dt, const void* dout, const void* out, const BnSide& a, const BnSide& b, float* partials, long npix, int C,
                         hipStream_t s);
// coefficients for dy = A*g + B*y + Cc, plus dgamma/dbeta (accumulated into grads with +=)
struct BnBwdFinalizeArgs {
  const float* partials; int nparts; int C; int which /*0: y0, 1: y1*/; int ny; double count;
  const float* gamma; const float* mean; const float* istd; float* dgamma; float* dbeta; float* coefA; float* coefB; float* coefC;
  // optional: bias gradient of the conv that feeds this BatchNorm, dbias[c] += dbias_scale * sum(dy) = A sum(g) + B sum(y) + C count
  // in closed form from the sums at hand (analytically zero: a bias in front of a BatchNorm has no gradient; what is left is the
  // rounding of the coefficients) -- no pass over dy, no atomics
  float* dbias_conv = nullptr; float dbias_scale = 1.f;
};
int launch_bn_bwd_finalize(const BnBwdFinalizeArgs& a, hipStream_t s);
int launch_bn_bwd_finalize2(const BnBwdFinalizeArgs& a0, const BnBwdFinalizeArgs& a1, hipStream_t s);   // two BNs of equal width, one launch
// dy0 = a.bwd(g, a.y) ; (dy1 = b.bwd(g, b.y) when b.y != null); the mask of g as in launch_bn_bwd_reduce
int launch_bn_bwd_apply(int dt, const void* dout, const void* out, const BnSide& a, const BnSide& b, void* dy0, void* dy1, long npix, int C,
                        hipStream_t s);
// NCHW f32 variants for the output BatchNorm (decoder.bn2): recon = raw*scale+shift ; backward pieces
int launch_affine_nchw(const float* raw, Affine bn, float* out, int N, int C, int HW, hipStream_t s);
int launch_bn_bwd_reduce_nchw(const float* dout, const float* y, int N, int C, int HW, float* partials, hipStream_t s);
int launch_bn_bwd_apply_nchw(const float* dout, const float* y, BnCoef k, float* dy, int N, int C, int HW, hipStream_t s);
// Gaussian NLL gradient fused into the output BatchNorm's backward: d = coef / sigma^2 * gscale[0] * (scale*raw + shift - target) is never stored
int launch_gauss_tail_reduce(const float* raw, Affine bn, const float* target, float sigma, float coef, const float* gscale, float* partials, int N,
                             int C, int HW, hipStream_t s);      // partial rows (sum d, sum d*raw); returns nparts
int launch_gauss_tail_apply(const float* raw, Affine bn, BnCoef k, const float* target, float sigma, float coef, const float* gscale, float* dy, int N,
                            int C, int HW, hipStream_t s);

// ---------------------------------------------------------------- last up-block: join + one-plane tail conv (tail_join.hip)
// y2 / ys: the block's two branch outputs under bn2 / the shortcut's BatchNorm; w: the tail conv's weights [OC][16][3][3] f32.
// Backward: the residual join's BatchNorm backward with the incoming gradient recomputed from the reconstruction gradient d_raw
bool tail_join_fusable(int dt, int OC, int N, int H, int W);
int launch_tail_join_bwd_reduce(int dt, const float* d_raw, const float* w, const BnSide& y2, const BnSide& ys, float* partials, int OC, int N,
                                int H, int W, hipStream_t s, float* wpartials = nullptr, int f8in = 0);
int launch_tail_wgrad_finalize(const float* wpartials, int nparts, float* dW, hipStream_t s);
int launch_tail_join_bwd_apply(int dt, const float* d_raw, const float* w, const BnSide& y2, const BnSide& ys, void* dy2, void* dys, int OC, int N,
                               int H, int W, hipStream_t s);
// Forward: residual join + tail conv in one pass, the joined activation is not stored
bool tail_fwd_fusable(int dt, int OC, int N, int H, int W);
int launch_tail_join_fwd(int dt, const BnSide& y2, const BnSide& ys, const float* w, const float* bias, float* r_raw, float* stats, int N, int H,
                         int W, hipStream_t s);

// ---------------------------------------------------------------- PixelCNN pieces (pixelcnn.hip; reference model.py:227-255)
// InstanceNorm2d (affine = False, eps 1e-5, instance statistics always) forward / backward fused with the ReLU behind it, and the layout
// changes between NCHW f32 and NHWC storage type with 16 zero-padded channels.  stats: [N][C][2] = (mean, istd).
int launch_inorm_planar_fwd(int dt, const float* x, void* xn16, float* stats, int N, int C, int HW, hipStream_t s);
// the same with the C = Ca + Cb channels taken from two tensors, xa [N][Ca][HW] then xb [N][Cb][HW] (either may be empty)
int launch_inorm_planar2_fwd(int dt, const float* xa, int Ca, const float* xb, int Cb, void* xn16, float* stats, int N, int HW, hipStream_t s);
int launch_inorm_planar_bwd(int dt, const void* g16, const float* x, const float* stats, float* dx, int N, int C, int HW, hipStream_t s);
int launch_inorm_nhwc_fwd(int dt, const void* h, void* a, float* stats, int N, int C, int HW, int relu, hipStream_t s);
int launch_inorm_nhwc_bwd(int dt, const void* g, const void* h, const float* stats, void* dh, int N, int C, int HW, int relu, hipStream_t s);
int launch_nhwc16_to_planar(int dt, const void* o16, float* out, int N, int C, int HW, hipStream_t s);
int launch_planar_to_nhwc16(int dt, const float* in, void* o16, int N, int C, int HW, hipStream_t s);
int launch_planar_to_nhwc16(int dt, const void* in, int in_dt, void* o16, int N, int C, int HW, hipStream_t s);

// One pixel of the autoregressive sampler (main.py:186-202): the last masked convolution at pixel `pix` = i * S + j only, softmax, the draw
// label = #{k <= Q - 2 : cdf_k <= uniforms[n][pix]} and sample[n][c][pix] = (label - sub_mean) / data_std for every sample channel c.
struct PixelHeadArgs {
  const void* a;             // [N][S][S][C] of T: the last layer's input
  const void* w;             // [>= Q][ntaps][C] of T: the last layer's weights as packed for the forward GEMM
  const float* bias;         // [Q]
  const float* uniforms;     // [N][S * S], in [0, 1)
  float* sample;             // [N][Cs][S][S]
  float* probs;              // [N][S * S][Q] or null
  long long* labels;         // [N][S * S] or null
  int S, C, Q, ntaps, Cs, pix;
  float sub_mean, data_std;
};
int launch_pixel_head(int dt, const PixelHeadArgs& h, int N, hipStream_t s);

// ---------------------------------------------------------------- latent / loss
// enc = mu + exp(0.5*logvar)*eps (f32 and T copies); kl_partial: -0.5*sum(lv - exp(lv) - mu^2 + 1) (one float, atomically added)
int launch_rsample_fwd(int dt, const float* mu, const float* logvar, const float* eps, float* enc_f32, void* enc_t, long n,
                       hipStream_t s);
int launch_rsample_bwd(const float* d_enc, const float* logvar, const float* eps, float* d_mu, float* d_logvar, long n, hipStream_t s);
// Every loss sum below adds into the f64 out[0] through `part` (MMVAE_SUM_PARTIALS doubles, part[0] zero between calls): a
// block-ordered reduction whose bits do not depend on block arrival order (latent_loss.hip); part == nullptr runs it in one block
int launch_kl_fwd(const float* mu, const float* logvar, long n, double* out, double* part, hipStream_t s);
// d_mu += coef*mu ; d_logvar += coef*0.5*(exp(lv)-1)   (coef = kl_weight * upstream / N)
int launch_kl_bwd(const float* mu, const float* logvar, float coef, const float* gscale, float* d_mu, float* d_logvar, long n, hipStream_t s);
// Gaussian NLL: out[0] += sum 0.5*((t-r)/sigma)^2 + log(sigma) + 0.5*log(2pi);  d_r = coef*(r-t)/sigma^2
int launch_gauss_nll_fwd(const float* r, const float* t, long n, float sigma, double* out, double* part, hipStream_t s);
int launch_gauss_nll_bwd(const float* r, const float* t, long n, float sigma, float coef, const float* gscale, float* d_r, hipStream_t s);
// weighted cross entropy over NCHW logits [N][Q][HW], int64 targets [N][HW]: out += sum w[t]*(log sum_q exp(r[q]-max) - (r[t]-max))
int launch_ce_fwd(const float* r, const long long* t, const float* w, int N, int Q, int HW, double* out, double* part, hipStream_t s);
int launch_ce_bwd(const float* r, const long long* t, const float* w, int N, int Q, int HW, float coef, const float* gscale, float* d_r,
                  hipStream_t s);
// MMD (sums): out += sum_ij k(x_i,x_j) + sum_ij k(y_i,y_j) - 2 sum_ij k(x_i,y_j), k = exp(-|a-b|^2/d^2)
int launch_mmd_fwd(const float* x, const float* y, int n, int d, double* out, double* part, hipStream_t s);
int launch_mmd_fwd_mfma(const float* x, const float* y, int n, int d, float* scratch /*2n floats*/, double* out, double* part, hipStream_t s);
// k[i][j] = exp(-|x_i - y_j|^2 / d^2), (n, m) f32  (VAE.compute_kernel, model.py:367-376)
int launch_rbf_matrix(const float* x, const float* y, int n, int m, int d, float* out, hipStream_t s);
// d_y[j] += coef * d(mmd)/d(y_j)
int launch_mmd_bwd(const float* x, const float* y, int n, int d, float coef, const float* gscale, float* d_y, hipStream_t s);

// ---------------------------------------------------------------- held-out evaluation (eval_loss.hip)
// Per-image f64 terms, out[n] WRITTEN by one block per image in a fixed order (no atomics); no alignment demanded of the rows.
// The callers (capi.cpp) have checked the arguments: N, per, Q, HW, d, K >= 1, no null pointer (weight excepted).
// out[n] = -sum_{i < per} log N(t[n][i]; r[n][i], sigma)
int launch_gauss_nll_per_image(const float* r, const float* t, int N, long per, float sigma, double* out, hipStream_t s);
// out[n] = sum_pix w[t] * (logsumexp_q r[n][:][pix] - r[n][t][pix]); w may be null
int launch_ce_per_image(const float* r, const long long* t, const float* w, int N, int Q, int HW, double* out, hipStream_t s);
// out[n] = -0.5 * sum_d (lv - exp(lv) - mu^2 + 1)
int launch_kl_per_image(const float* mu, const float* logvar, int N, int d, double* out, hipStream_t s);
// out[n] = log p(z) - log q(z|x) = -0.5 * sum_d (z^2 - eps^2 - lv), z = mu + exp(lv/2) * eps as launch_rsample_fwd forms it
int launch_latent_logratio(const float* mu, const float* logvar, const float* eps, int N, int d, double* out, hipStream_t s);
// nll, logratio f64 [K][N]: out[n] = logsumexp_k(logratio[k][n] - nll[k][n]) - log K
int launch_iw_bound(const double* nll, const double* logratio, int K, int N, double* out, hipStream_t s);

// ---------------------------------------------------------------- optimiser / misc
struct AdamArgs { float* p; const float* g; float* m; float* v; long n; float lr, beta1, beta2, eps, weight_decay; float bc1, bc2; float grad_scale; };
int launch_adam(const AdamArgs& a, hipStream_t s);
int launch_adam_dev(const AdamArgs& a, double* state, hipStream_t s);   // step count on the device (graph capture): bc1 / bc2 ignored
// acc[0] += sum (g[i] * grad_scale)^2 in f64 through `part` (as the loss sums above; nullptr: one block); any alignment of g
int launch_grad_norm_sq(const float* g, long n, float grad_scale, double* acc, double* part, hipStream_t s);
// launch_adam_dev behind a global-norm clip (max_norm > 0) and a skip of non-finite steps; state = {step count, total norm of the last
// call, skipped steps, norm^2 accumulator (zero between calls)}
int launch_adam_guarded(const AdamArgs& a, double* state, double* part, float max_norm, hipStream_t s);
// labels (int64) -> image T [(l - mean)/std] (+ f32 copy for the Gaussian target)
// labels: int64 (label_bytes = 8) or uint8 (1)
int launch_normalise(int dt, const void* labels, int label_bytes, long n, float mean, float stdv, void* img_t, float* img_f32, hipStream_t s);
int launch_quantise_normalise(const unsigned char* frames, long n, const float* centres, int q, float mean, float stdv,
                              long long* labels, float* image, hipStream_t s);
// counts[b] += occurrences of byte b in n_clips ranges of clip_bytes bytes: frames + clip_index[i] * clip_bytes, or the contiguous
// [0, n_clips * clip_bytes) with clip_index == nullptr (quantiser.hip); any alignment of frames and clip_bytes
int launch_u8_histogram(const unsigned char* frames, long clip_bytes, const long long* clip_index, long n_clips,
                        unsigned long long* counts, hipStream_t s);
// Pillow's 8-bit antialiased bilinear resize of n_frames uint8 planes (horizontal pass first) fused with the quantiser above
// (resize.hip); tables from resample_coeffs, on the device.  Plane p is plane p % frames_per_clip of clip clip_index[p / frames_per_clip]
// (or of clip p / frames_per_clip), planes frame_stride bytes apart; outputs are dense, any of them may be null but not all
int launch_resize_quantise_normalise(const unsigned char* frames, long frame_stride, const long long* clip_index, int frames_per_clip,
                                     long n_frames, int in_h, int in_w, int out_h, int out_w, const int* h_bounds, const int* h_coeffs,
                                     int h_ksize, const int* v_bounds, const int* v_coeffs, int v_ksize, const float* centres, int q,
                                     float mean, float stdv, long long* labels, float* image, unsigned char* resized, hipStream_t s);
// Moving MNIST clips first_clip .. first_clip + n_clips - 1 by the integer rule of mmvae.h (clipgen.hip), written as the quantiser's
// outputs (labels, image) and / or the bytes, dense [n_clips][T][S][S]; any of the three may be null but not all.  vel: device int32
// [4096][2].  Checks its arguments before anything is enqueued.
constexpr int kClipGenMaxG = MMVAE_CLIPGEN_MAX_G, kClipGenMaxT = MMVAE_CLIPGEN_MAX_T, kClipGenMaxK = MMVAE_CLIPGEN_MAX_K;
constexpr long kClipGenMaxD = MMVAE_CLIPGEN_MAX_D;
int launch_generate_clips(const unsigned char* bank, long D, int G, const int* vel, unsigned long long seed, long first_clip, long n_clips,
                          int T, int S, int K, const float* centres, int q, float mean, float stdv, long long* labels, float* image,
                          unsigned char* bytes, hipStream_t s);
// picture panels (panels.hip): logits [N][Q][HW] -> labels by the shared pick rule (mode: MMVAE_PICK_*), and a whole uint8 contact sheet
// [n * S][ncols * S] from ncols column descriptors (host array, passed to the kernel by value)
int launch_logits_to_labels(const float* logits, int N, int Q, int HW, int mode, const float* uniforms, long long* labels, hipStream_t s);
int launch_panel_sheet(const mmvae_panel_col* cols, int ncols, int n, int S, unsigned char* out, hipStream_t s);
// per-frame quality (frame_quality.hip): out f64 [2][n] = squared error and SSIM (11 x 11 Gaussian window, valid positions) of n pairs of
// S x S planes, each side one column descriptor reduced to bytes by the sheet's rule (or MMVAE_FRAME_BYTES_U8); 11 <= S <= 64
int launch_frame_quality(const mmvae_panel_col* a, const mmvae_panel_col* b, int n, int S, double* out, hipStream_t s);
// latent diagnostics (latent_diag.hip): the density panel of n 2-D points pts[p * stride + col_x / col_y] (xform: device {xlim, ylim, sx, sy};
// byte = tone[min(#covering discs, 255)], out rows out_row_stride bytes apart), and acc[6][d] f64 per-dimension sums over N images of
// mu, mu^2, the KL term, exp(logvar), enc, enc^2 (logvar / enc nullable: their rows are zero; accumulate: add to acc instead of writing).
// Both check their arguments before anything is enqueued.
int launch_scatter_panel(const float* pts, long n, int stride, int col_x, int col_y, const float* xform, int side, int radius16,
                         const unsigned char* tone, unsigned char* out, long out_row_stride, hipStream_t s);
int launch_latent_stats(const float* mu, const float* logvar, const float* enc, int N, int d, int accumulate, double* acc, hipStream_t s);
// aggregate-posterior densities (posterior_mixture.hip): log_qz[N] and (nullable) log_qz_dims[N][d] f64 = logsumexp over the M bank
// posteriors (mu, logvar [M][d]) of the joint / per-dimension Gaussian log-density of z [N][d], minus log M.  The scratch size is a
// function of the shape alone (0 for a shape the launcher refuses); both check their arguments before anything is enqueued.
size_t posterior_mixture_scratch_bytes(int N, int M, int d);
int launch_posterior_mixture(const float* z, int N, const float* mu, const float* logvar, int M, int d, double* log_qz, double* log_qz_dims,
                             void* scratch, size_t scratch_bytes, hipStream_t s);
// their gradient (posterior_mixture_bwd.hip): d_z [N][d], d_mu, d_logvar [M][d] f32 from the saved outputs and the upstream gradients
// g_joint [N], g_dims [N][d] f64 (either nullable, not both; log_qz_dims nullable with g_dims).  Written, not accumulated; N, M <= 16384.
size_t posterior_mixture_bwd_scratch_bytes(int N, int M, int d);
int launch_posterior_mixture_bwd(const float* z, int N, const float* mu, const float* logvar, int M, int d, const double* log_qz,
                                 const double* log_qz_dims, const double* g_joint, const double* g_dims, float* d_z, float* d_mu,
                                 float* d_logvar, void* scratch, size_t scratch_bytes, hipStream_t s);
// exact k nearest frames of M uint8 query planes among F frames of D bytes (neighbours.hip): squared distances in integers, ties to the
// lower frame index, lut (nullable, 256 device bytes) applied to the frames only.  The scratch size is a function of the shape alone
// (0 for a shape the launcher refuses); both check their arguments before anything is enqueued.
size_t nearest_frames_scratch_bytes(int M, long F, int D, int k);
int launch_nearest_frames(const unsigned char* queries, int M, const unsigned char* frames, long F, int D, const unsigned char* lut, int k,
                          int* out_dist, long long* out_index, void* scratch, size_t scratch_bytes, hipStream_t s);
// set-to-set exact k-NN and ball counts (knn_cross.hip): every row of a [Na][D] uint8 against every row of b [Nb][D] uint8, the k smallest
// (d, j) per row of a (k = 0: none) and / or #{ j : d(i, j) <= col_radius[j] } (col_radius and out_count both NULL: none);
// exclude_diagonal drops the pairs (i, i).  The scratch size is a function of the shape alone (0 for a shape the launcher refuses);
// both check their arguments before anything is enqueued.
size_t knn_cross_scratch_bytes(long Na, long Nb, int D, int k, int want_count);
int launch_knn_cross(const unsigned char* a, long Na, const unsigned char* b, long Nb, int D, int k, int exclude_diagonal, int* out_dist,
                     long long* out_index, const int* col_radius, int* out_count, void* scratch, size_t scratch_bytes, hipStream_t s);
// 64-bin histograms and exact statistics of T segments (offset, numel) of a flat f32 buffer (tensor_hist.hip), work cut into chunks
// (segment, start, length).  seg_host / chunk_host are checked before anything is enqueued, seg_dev / chunk_dev are what the kernels read.
long long tensor_hist_chunks(const long long* segments, int T, long long chunk_elems, long long* chunks, long long capacity);
size_t tensor_hist_scratch_bytes(int T, long long n_chunks);
int launch_tensor_hist(const float* flat, long long flat_numel, const long long* seg_host, const long long* seg_dev, int T,
                       const long long* chunk_host, const long long* chunk_dev, long long n_chunks, int* counts, float* lo, float* hi,
                       double* stats, void* scratch, size_t scratch_bytes, hipStream_t s);
int launch_convert(int dt_in, int dt_out, const void* in, void* out, long n, hipStream_t s);
int launch_fill_f32(float* p, float v, long n, hipStream_t s);
int launch_concat2_to_t(int dt, const float* a, const float* b, int rows, int ca, int cb, void* out, hipStream_t s);
int launch_loss_finish(const double* acc, float* out, float nll, float klc, float mmdc, float n, hipStream_t s);
// out[c] += sum_p partials[p*row_stride + c]  (c < C)
int launch_partials_add(const float* partials, int nparts, int row_stride, int C, float* out, hipStream_t s);

}  // namespace mmvae
