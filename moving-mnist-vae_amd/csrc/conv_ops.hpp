// Geometry-level conv operations shared by the network orchestrator and the single-op C ABI.
// A conv-like weight [D0][D1][k][k] relates a "small" tensor S [N,Hs,Ws,D0] and a "large" tensor L [N,Hl,Wl,D1]
// with Hs = floor((Hl + 2p - k)/s) + 1:
//   Conv2d          weight (out,in,k,k):  forward = down(L->S), dgrad = up(S->L),   wgrad(P = dy (S), G = x (L))
//   ConvTranspose2d weight (in,out,k,k):  forward = up(S->L),   dgrad = down(L->S), wgrad(P = x (S),  G = dy (L))
#pragma once
#include "kernels.hpp"

namespace mmvae {

struct ConvGeom { int D0, D1, k, s, p; };

inline int conv_down_size(int H, int k, int s, int p) { return (H + 2 * p - k) / s + 1; }
// packed element counts (both equal numel(weight)); 16-byte alignment is the caller's job
// scale multiplies the weights (fp8 layers: the static per-layer scale); fp8 = 1 writes e4m3 bytes (batched packing only)
// frag = 1: fragment-major order (PackArgs::frag) -- what deep2_conv_kernel and pos_conv_kernel read; op_down_layout / op_up_layout say
// whether to pack and run with the flag set.
int op_pack_down(int dt, const ConvGeom& g, const float* w, void* dst, hipStream_t s, float scale = 1.f, int fp8 = 0, int frag = 0);
int op_pack_up(int dt, const ConvGeom& g, const float* w, void* dst, hipStream_t s, float scale = 1.f, int fp8 = 0, int frag = 0);
// Where the run_down / run_up launch of this geometry (large-side map Hl x Wl) goes, asked of the dispatcher itself with the launch's own
// GatherArgs (gather_deep2_takes / gather_pos_takes, kernels.hpp):
struct ConvLayout {
  bool frag = false;   // deep2_conv_kernel takes it: pack fragment-major and run with wfrag set
  bool fp8 = false;    // the e4m3 form of deep2_conv_kernel takes it (bf16 storage, non-accumulating launches)
  bool pos = false;    // with fragment-major bf16 weights the position-major kernel, which is offered the launch first, takes it
};
ConvLayout op_down_layout(int dt, const ConvGeom& g, int Hl, int Wl);
// allow_empty_phases: the launch accumulates (or is a second source), so stride phases without a tap are skipped, not zero-filled
ConvLayout op_up_layout(int dt, const ConvGeom& g, int Hl, int Wl, int allow_empty_phases = 0);
// x2 / w2 / Cin2 (optional): a second tensor on the q grid (= S for run_down, = the S-resolution grid for run_up) whose 1x1
// convolution with the packed [Cout][Cin2] matrix w2 is added into the result (phase (0,0) of run_up) in the same kernel.
struct SecondSrc {
  const void* x2 = nullptr; const void* w2 = nullptr; int Cin2 = 0;
  int fp8 = 0;             // the forward conv runs on the fp8 MFMA (e4m3 packed weights)
  int wfrag = 0, wfrag2 = 0;   // packed (w2) is fragment-major
};
// Every op below takes one operand per tensor (MapIn / MapOut, kernels.hpp) in one order: the packed weights, the input maps, the outputs, the
// batch size, the stream, then defaulted options.  The shape predicates ask with the same operands and no data (MapIn::shape).
int op_run_down(int dt, int out_dt, const ConvGeom& g, const void* packed, const MapIn& L, const MapOut& S, int N, hipStream_t s,
                const SecondSrc& x2 = SecondSrc());
int op_run_up(int dt, const ConvGeom& g, const void* packed, const MapIn& S, const MapOut& L, int N, hipStream_t s,
              const SecondSrc& x2 = SecondSrc());      // L.accumulate: stride phases without a tap are skipped, not zero-filled
// The builders behind them, for the launches that differ from a layer's own in a few fields (boundary layers, PixelCNN): the GatherArgs / WgradArgs
// of the geometry without data pointers and per-call options; false: the geometry has no launch.  ntaps > 0 (down form): only the first
// ntaps taps, row-major (a masked kernel; wgrad_args likewise).  up_args' skip_empty: stride phases without a tap are left out instead of zero-filled.
bool down_args(GatherArgs& a, const ConvGeom& g, int N, int Hl, int Wl, int Hs, int Ws, int ntaps = 0);
bool up_args(GatherArgs& a, const ConvGeom& g, int N, int Hs, int Ws, int Hl, int Wl, bool skip_empty);
void wgrad_args(WgradArgs& a, const ConvGeom& g, int N, const MapIn& P, const MapIn& G, float* dW, float* scratch, float scale = 1.f, int ntaps = 0);

// options of the weight-gradient ops; the second group is op_run_bwd_fused's (op_run_wgrad_pair reads scale2)
struct WgradOpts {
  float* scratch = nullptr;            // kWgradScratchBytes, not shared with a concurrent wgrad
  float scale = 1.f;
  WgradReduceArgs* defer = nullptr;    // WgradArgs::defer
  float* bn_part = nullptr;            // (P prologue'd, no x2) the pass also leaves the BatchNorm-backward partial sums of P's BatchNorm, rows
                                       // [return value][2][16] -- the layout launch_bn_bwd_reduce writes
  float* dW2 = nullptr; float scale2 = 1.f;   // (with x2) the 1x1 conv's own weight gradient [16][D0] row-major (Conv2d (out, in, 1, 1)) += scale2 * x2^T (x) pro(P)
  const BnSide* jg = nullptr;          // G is the masked gradient of a residual join's output and the layer's dy is evaluated on load (kernels.hpp,
                                       // try_dgrad_wgrad_stream) -- no bn_bwd_apply pass, no dy tensor
};
int op_run_wgrad(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, float* dW, int N, hipStream_t s, const WgradOpts& o = WgradOpts());
bool op_wgrad_is_stream(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, int N);
// P2 / dW2: the shortcut's dy on P's grid and its weight gradient
int op_run_wgrad_pair(int dt, const ConvGeom& g, const ConvGeom& gs, const MapIn& P, const void* P2, const MapIn& G, float* dW, float* dW2, int N,
                      hipStream_t s, const WgradOpts& o);

bool op_bwd_fusable(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, int N);
// Weight gradient AND the data gradient w.r.t. the small-side tensor P in ONE pass over G (wgrad_stream_kernel with DG; the 16 -> 16
// channel k4 s2 layers on 32x32 -> 64x64 maps, bf16):  dW += P^T (x) G;  dP = down(G) with the conv's packed down form (+ x2.x2 (x) x2.w2,
// the 1x1 shortcut's share, x2 on P's grid with 16 channels, w2 its packed up form).  Returns 1 when taken, 0 when the shape is not
// that kernel's (callers then run op_run_down + op_run_wgrad), <0 on error.  With o.bn_part, taken: returns the number of rows (> 0).
int op_run_bwd_fused(int dt, const ConvGeom& g, const void* packed_down, const MapIn& P, const MapIn& G, const SecondSrc& x2, void* dP, float* dW, int N,
                     hipStream_t s, const WgradOpts& o);
// whether op_run_bwd_fused takes this layer with a join gradient o.jg (16-wide maps; conv2 with prologue + BatchNorm sums, or the 32-channel
// shortcut with the 1x1 conv's second source)
bool op_bwd_fusable_jg(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, int N, bool has_x2, bool bn_sums);

// ---- boundary-layer pieces shared by the network and the single-op C ABI
// A 3x3 Conv2d weight (Cout,Cin,3,3) packed [cin][flipped tap][cout]: its stride-1 data gradient is then a forward conv over dy
// (dx[n,h,w,ci] = sum_{kh,kw,co} dy[n, h+1-kh, w+1-kw, co] W[co][ci][kh][kw], tap' = 8 - tap)
int op_pack_flipped3(int dt, const float* w, void* dst, int Cin, int Cout, hipStream_t s, float scale = 1.f);
// stem Conv2d(in_ch -> 32, k5 s2 p2) where the stream kernel does not take it: the weights [32][25][one vector of zero-padded input channels], and
// the planar image (in_ch <= 4 planes of S x S) through the patch-tile kernel, which stages it as that many NHWC channels in LDS
int op_pack_stem(int dt, const float* w, int in_ch, void* dst, hipStream_t s);
int op_run_stem(int dt, const void* packed, const void* x, int in_ch, int S, const MapOut& y, int N, hipStream_t s);

}  // namespace mmvae
