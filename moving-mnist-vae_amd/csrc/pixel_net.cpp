// PixelCNN (reference model.py:227-255: InstanceNorm -> [MaskedConv2d 7x7 -> InstanceNorm -> ReLU] x (layers - 1) -> MaskedConv2d 7x7)
// forward and backward on the generic convolution kernels: a type-A / type-B mask keeps the first 24 / 25 taps of the 7x7 kernel in
// row-major order (model.py:216-220), so every layer is a stride-1 convolution with that tap list -- the masked taps are never packed,
// multiplied or differentiated.  Activations: NHWC storage type, channel counts padded to multiples of 16 at the two boundaries
// (pixelcnn.hip converts from / to the reference's NCHW f32 tensors).  Owns no tensors: parameters, gradients and the workspace are the
// caller's.  Not a benchmarked path: correctness first, no fusion beyond InstanceNorm + ReLU.
#include "pixel_net.hpp"

#include <cstring>

#include "conv_ops.hpp"

namespace mmvae {

#define MM_TRY(expr)            \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ < 0) return rc__;  \
  } while (0)

static inline long align_up(long v, long a) { return (v + a - 1) / a * a; }
static inline int pad16(int c) { return (c + 15) / 16 * 16; }

PixelNet::PixelNet(int in_ch_, int mid_, int out_ch_, int layers_, int dtype_) : in_ch(in_ch_), mid(mid_), out_ch(out_ch_), layers(layers_), dtype(dtype_) {
  long off = 0, poff = 0;
  for (int i = 0; i < layers; ++i) {
    Layer L;
    L.cin = i == 0 ? in_ch : mid; L.cout = i == layers - 1 ? out_ch : mid;
    L.cin_p = i == 0 ? pad16(in_ch) : mid; L.cout_p = i == layers - 1 ? pad16(out_ch) : mid;
    L.ntaps = i == 0 ? 24 : 25;                                   // type A: rows 0..2 and 3 taps of row 3; type B: + the centre
    L.w_off = off; off += (long)L.cout * L.cin * 49;
    L.b_off = off; off += L.cout;
    L.packF = poff; poff += align_up((long)L.cout_p * L.ntaps * L.cin_p, 8);
    L.packB = poff; poff += align_up((long)L.cin_p * L.ntaps * L.cout_p, 8);
    lay.push_back(L);
  }
  n_params = off; n_packed = poff;
}

const PixelPlan& PixelNet::plan(int N, int S) {
  if (plan_.N == N && plan_.S == S) return plan_;
  PixelPlan P; P.N = N; P.S = S;
  const long e = (long)dtype_size(dtype), HW = (long)S * S;
  long cur = 0;
  auto take = [&](long bytes) { long o = cur; cur = align_up(cur + (bytes > 16 ? bytes : 16), 256); return o; };
  P.x0 = take((long)N * HW * lay[0].cin_p * e);
  P.st0 = take((long)N * in_ch * 2 * 4);
  for (int i = 0; i < layers; ++i) {
    P.h[i] = take((long)N * HW * lay[i].cout_p * e);
    if (i < layers - 1) { P.a[i] = take((long)N * HW * mid * e); P.st[i] = take((long)N * mid * 2 * 4); }
  }
  P.g[0] = take((long)N * HW * (mid > 16 ? mid : 16) * e);
  P.g[1] = take((long)N * HW * (mid > 16 ? mid : 16) * e);
  P.packed = take(n_packed * e);
  P.bias_pad = take(16 * 4);
  P.partials = take(1024L * 2 * 256 * 4);
  P.wscratch = take((long)kWgradScratchBytes);
  P.bytes = (size_t)cur;
  plan_ = P;
  return plan_;
}

// A layer is a 7x7 stride-1 pad-3 conv masked to its first ntaps taps, t = 7 kh + kw: forward offset (kh - 3, kw - 3) -- down_args' order --,
// data gradient the mirrored one
static inline ConvGeom geom7(int D0, int D1) { return ConvGeom{D0, D1, 7, 1, 3}; }

int PixelNet::pack(const float* params, char* base, bool data_grad, hipStream_t s) {
  const PixelPlan& P = plan_;
  const long e = (long)dtype_size(dtype);
  pack_batch_begin();
  for (const Layer& L : lay) {
    PackArgs f; std::memset(&f, 0, sizeof(f));     // forward: [cout_p][tap][cin_p]
    f.src = params + L.w_off; f.dst = base + P.packed + L.packF * e;
    f.cols = L.cout_p; f.cols_valid = L.cout; f.K = L.cin_p; f.K_valid = L.cin; f.ntaps = L.ntaps; f.s_col = L.cin * 49; f.s_k = 49; f.scale = 1.f;
    for (int t = 0; t < L.ntaps; ++t) f.tap_off[t] = t;
    MM_TRY(launch_pack(dtype, f, s));
    if (!data_grad) continue;
    PackArgs b; std::memset(&b, 0, sizeof(b));     // data gradient: [cin_p][tap][cout_p]
    b.src = params + L.w_off; b.dst = base + P.packed + L.packB * e;
    b.cols = L.cin_p; b.cols_valid = L.cin; b.K = L.cout_p; b.K_valid = L.cout; b.ntaps = L.ntaps; b.s_col = 49; b.s_k = L.cin * 49; b.scale = 1.f;
    for (int t = 0; t < L.ntaps; ++t) b.tap_off[t] = t;
    MM_TRY(launch_pack(dtype, b, s));
  }
  return pack_batch_flush(dtype, s);
}

// layer i over the full map: h[i] = conv(x) + bias (model.py:223)
int PixelNet::conv(int i, int N, int S, const void* x, const float* params, char* base, hipStream_t s) {
  const PixelPlan& P = plan_;
  const Layer& L = lay[i];
  const long e = (long)dtype_size(dtype);
  float* bias = const_cast<float*>(params) + L.b_off;
  if (L.cout_p != L.cout) {     // last layer: the bias vector padded with zeros to the GEMM's 16 rows
    bias = reinterpret_cast<float*>(base + P.bias_pad);
    MM_TRY(launch_fill_f32(bias, 0.f, 16, s));
    if (hipMemcpyAsync(bias, params + L.b_off, (size_t)L.cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) { set_error("pixelcnn: bias copy failed"); return MMVAE_ERR_HIP; }
  }
  GatherArgs a;
  down_args(a, geom7(L.cout_p, L.cin_p), N, S, S, S, S, L.ntaps);
  a.x = x; a.w = base + P.packed + L.packF * e; a.y = base + P.h[i]; a.bias = bias;
  return launch_gather_gemm(dtype, dtype, a, s);
}

// layers 0 .. layers - 2 on the instance-normalised input in x0; returns the last layer's input
int PixelNet::trunk(int N, int S, const float* params, char* base, const void** last_in, hipStream_t s) {
  const PixelPlan& P = plan_;
  const void* cur = base + P.x0;
  for (int i = 0; i < layers - 1; ++i) {
    MM_TRY(conv(i, N, S, cur, params, base, s));
    MM_TRY(launch_inorm_nhwc_fwd(dtype, base + P.h[i], base + P.a[i], reinterpret_cast<float*>(base + P.st[i]), N, mid, S * S, 1, s));   // model.py:252-253
    cur = base + P.a[i];
  }
  *last_in = cur;
  return MMVAE_OK;
}

int PixelNet::forward(int N, int S, const float* x, const float* params, void* ws, size_t ws_bytes, float* out, hipStream_t s) {
  const PixelPlan& P = plan(N, S);
  if (ws_bytes < P.bytes) { set_error("pixelcnn: workspace too small: %zu < %zu", ws_bytes, P.bytes); return MMVAE_ERR_WORKSPACE; }
  char* base = static_cast<char*>(ws);
  const int HW = S * S;
  MM_TRY(pack(params, base, true, s));
  MM_TRY(launch_inorm_planar_fwd(dtype, x, base + P.x0, reinterpret_cast<float*>(base + P.st0), N, in_ch, HW, s));      // model.py:249
  const void* cur = nullptr;
  MM_TRY(trunk(N, S, params, base, &cur, s));
  MM_TRY(conv(layers - 1, N, S, cur, params, base, s));
  return launch_nhwc16_to_planar(dtype, base + P.h[layers - 1], out, N, out_ch, HW, s);
}

// The autoregressive sampling loop of main.py:186-202, enqueued whole: per pixel, InstanceNorm of (cond, sample), layers 0 .. layers - 2
// over the full map (their InstanceNorms see every pixel, so nothing of them can be cached) and the head kernel, which evaluates the
// last layer at that pixel, draws and writes the sample in place: 2 (layers - 1) + 2 launches per pixel, no allocation, copy or host
// read.  The weights are packed once.  out (nullable): the logits of the last full forward, i.e. on the sample as it was before the last
// pixel was written (what the reference's loop returns).
int PixelNet::sample(int N, int S, const float* cond, int cond_ch, float* smp, int smp_ch, const float* uniforms, float sub_mean, float data_std,
                     const float* params, void* ws, size_t ws_bytes, float* out, float* probs, long long* labels, hipStream_t s) {
  if (cond_ch < 0 || smp_ch < 1 || cond_ch + smp_ch != in_ch) {
    set_error("pixelcnn_sample: %d conditioning + %d sample channels, the net takes %d", cond_ch, smp_ch, in_ch);
    return MMVAE_ERR_ARG;
  }
  if (cond_ch > 0 && !cond) { set_error("pixelcnn_sample: %d conditioning channels but no conditioning image", cond_ch); return MMVAE_ERR_ARG; }
  if (!(data_std != 0.f)) { set_error("pixelcnn_sample: data_std must not be zero"); return MMVAE_ERR_ARG; }
  const PixelPlan& P = plan(N, S);
  if (ws_bytes < P.bytes) { set_error("pixelcnn_sample: workspace too small: %zu < %zu", ws_bytes, P.bytes); return MMVAE_ERR_WORKSPACE; }
  char* base = static_cast<char*>(ws);
  const int HW = S * S;
  const Layer& L = lay[layers - 1];
  MM_TRY(pack(params, base, false, s));
  PixelHeadArgs h; std::memset(&h, 0, sizeof(h));
  h.w = base + P.packed + L.packF * (long)dtype_size(dtype); h.bias = params + L.b_off; h.uniforms = uniforms;
  h.sample = smp; h.probs = probs; h.labels = labels;
  h.S = S; h.C = L.cin_p; h.Q = L.cout; h.ntaps = L.ntaps; h.Cs = smp_ch; h.sub_mean = sub_mean; h.data_std = data_std;
  for (int pix = 0; pix < HW; ++pix) {
    MM_TRY(launch_inorm_planar2_fwd(dtype, cond, cond_ch, smp, smp_ch, base + P.x0, reinterpret_cast<float*>(base + P.st0), N, HW, s));
    MM_TRY(trunk(N, S, params, base, &h.a, s));
    if (pix == HW - 1 && out) {
      MM_TRY(conv(layers - 1, N, S, h.a, params, base, s));
      MM_TRY(launch_nhwc16_to_planar(dtype, base + P.h[layers - 1], out, N, out_ch, HW, s));
    }
    h.pix = pix;
    MM_TRY(launch_pixel_head(dtype, h, N, s));
  }
  return MMVAE_OK;
}

int PixelNet::backward(int N, int S, const float* x, const float* d_out, const float* params, float* grads, void* ws, size_t ws_bytes, float* d_x,
                       hipStream_t s) {
  const PixelPlan& P = plan(N, S);
  if (ws_bytes < P.bytes) { set_error("pixelcnn: workspace too small"); return MMVAE_ERR_WORKSPACE; }
  char* base = static_cast<char*>(ws);
  const int HW = S * S;
  const long e = (long)dtype_size(dtype);
  float* part = reinterpret_cast<float*>(base + P.partials);
  float* wsc = reinterpret_cast<float*>(base + P.wscratch);
  // gradient w.r.t. the last conv's output, padded to 16 channels
  MM_TRY(launch_planar_to_nhwc16(dtype, d_out, base + P.g[0], N, out_ch, HW, s));
  int cur = 0;
  for (int i = layers - 1; i >= 0; --i) {
    const Layer& L = lay[i];
    const void* dy = base + P.g[cur];                         // [N][S][S][cout_p]
    const void* xin = i == 0 ? base + P.x0 : base + P.a[i - 1];
    // bias gradient: per-channel sums of dy
    {
      const int np = launch_chan_stats_nhwc(dtype, dy, (long)N * HW, L.cout_p, part, s);
      MM_TRY(np);
      MM_TRY(launch_partials_add(part, np, 2 * L.cout_p, L.cout, grads + L.b_off, s));
    }
    // weight gradient over the layer's taps: dW[co][ci][t] += sum_pix dy[pix][co] * x[pix + off_t][ci]
    {
      WgradArgs w;      // the unpadded weight's strides, its real channels, the mask's taps
      wgrad_args(w, geom7(L.cout_p, L.cin_p), N, MapIn(dy, S, S), MapIn(xin, S, S), grads + L.w_off, wsc, 1.f, L.ntaps);
      w.Ca_valid = L.cout; w.Cb_valid = L.cin; w.sA = L.cin * 49;
      MM_TRY(launch_wgrad(dtype, w, s));
    }
    if (i == 0 && !d_x) break;
    // data gradient: dx[pix][ci] = sum_t sum_co dy[pix - off_t][co] * W[co][ci][t]
    {
      GatherArgs a;
      down_args(a, geom7(L.cin_p, L.cout_p), N, S, S, S, S, L.ntaps);
      for (int t = 0; t < L.ntaps; ++t) a.taps[t] = Tap{-a.taps[t].dh, -a.taps[t].dw};
      a.x = dy; a.w = base + P.packed + L.packB * e; a.y = base + P.g[cur ^ 1];
      MM_TRY(launch_gather_gemm(dtype, dtype, a, s));
    }
    cur ^= 1;
    if (i > 0) {
      // InstanceNorm + ReLU backward of layer i - 1's output (in place on the gradient buffer is not possible: g and dh differ per element only)
      MM_TRY(launch_inorm_nhwc_bwd(dtype, base + P.g[cur], base + P.h[i - 1], reinterpret_cast<const float*>(base + P.st[i - 1]), base + P.g[cur ^ 1], N, mid, HW,
                                   1, s));
      cur ^= 1;
    } else {
      MM_TRY(launch_inorm_planar_bwd(dtype, base + P.g[cur], x, reinterpret_cast<const float*>(base + P.st0), d_x, N, in_ch, HW, s));
    }
  }
  return MMVAE_OK;
}

}  // namespace mmvae
