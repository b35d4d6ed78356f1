#include "conv_ops.hpp"

#include <cstdlib>
#include <cstring>

namespace mmvae {

#define MM_TRY(expr)            \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ < 0) return rc__;  \
  } while (0)

// stride phases of an "up" (transposed) gather: for output phase (ph,pw) the kernel taps with (ph+p-kh) % s == 0
struct UpPhase { int ph, pw; int ntaps; int kh[16], kw[16], dh[16], dw[16]; };
static int up_phases(int k, int s, int p, UpPhase* out) {
  int n = 0;
  for (int ph = 0; ph < s; ++ph)
    for (int pw = 0; pw < s; ++pw) {
      UpPhase& u = out[n++];
      u.ph = ph; u.pw = pw; u.ntaps = 0;
      for (int kh = 0; kh < k; ++kh) {
        const int th = ph + p - kh;
        if (((th % s) + s) % s != 0) continue;
        for (int kw = 0; kw < k; ++kw) {
          const int tw = pw + p - kw;
          if (((tw % s) + s) % s != 0) continue;
          u.kh[u.ntaps] = kh; u.kw[u.ntaps] = kw;
          u.dh[u.ntaps] = th / s; u.dw[u.ntaps] = tw / s;   // exact divisions
          ++u.ntaps;
        }
      }
    }
  return n;
}

int op_pack_down(int dt, const ConvGeom& g, const float* w, void* dst, hipStream_t s, float scale, int fp8, int frag) {
  PackArgs a; std::memset(&a, 0, sizeof(a));
  const int kk = g.k * g.k;
  if (kk > kMaxTaps) { set_error("pack_down: k=%d too large", g.k); return MMVAE_ERR_UNSUPPORTED; }
  a.src = w; a.dst = dst;
  a.cols = g.D0; a.K = g.D1; a.ntaps = kk; a.s_col = g.D1 * kk; a.s_k = kk; a.scale = scale; a.fp8 = fp8; a.frag = frag;
  for (int t = 0; t < kk; ++t) a.tap_off[t] = t;
  return launch_pack(dt, a, s);
}

int op_pack_up(int dt, const ConvGeom& g, const float* w, void* dst, hipStream_t s, float scale, int fp8, int frag) {
  if (g.s > 2 || g.k * g.k > kMaxTaps) { set_error("pack_up: k=%d s=%d unsupported", g.k, g.s); return MMVAE_ERR_UNSUPPORTED; }
  UpPhase ph[4];
  const int np = up_phases(g.k, g.s, g.p, ph);
  const int kk = g.k * g.k;
  const long e = fp8 ? 1 : (long)dtype_size(dt);
  long off = 0;
  for (int i = 0; i < np; ++i) {
    if (ph[i].ntaps == 0) continue;
    PackArgs a; std::memset(&a, 0, sizeof(a));
    a.src = w; a.dst = static_cast<char*>(dst) + off * e;
    a.cols = g.D1; a.K = g.D0; a.ntaps = ph[i].ntaps; a.s_col = kk; a.s_k = g.D1 * kk; a.scale = scale; a.fp8 = fp8; a.frag = frag;
    for (int t = 0; t < ph[i].ntaps; ++t) a.tap_off[t] = ph[i].kh[t] * g.k + ph[i].kw[t];
    MM_TRY(launch_pack(dt, a, s));
    off += (long)g.D1 * ph[i].ntaps * g.D0;
  }
  return MMVAE_OK;
}

void wgrad_args(WgradArgs& a, const ConvGeom& g, int N, const MapIn& P, const MapIn& G, float* dW, float* scratch, float scale, int ntaps) {
  std::memset(&a, 0, sizeof(a));
  const int kk = g.k * g.k;
  if (ntaps <= 0) ntaps = kk;
  a.P = P.x; a.G = G.x; a.dW = dW; a.scratch = scratch;
  a.proP_scale = P.pro.scale; a.proP_shift = P.pro.shift; a.proP_relu = P.relu;
  a.proG_scale = G.pro.scale; a.proG_shift = G.pro.shift; a.proG_relu = G.relu;
  a.N = N; a.Hp = P.H; a.Wp = P.W; a.Ca = g.D0; a.Hg = G.H; a.Wg = G.W; a.Cb = g.D1; a.Cb_valid = g.D1; a.Ca_valid = g.D0;
  a.stride = g.s; a.pad = g.p; a.ksz = g.k; a.sA = g.D1 * kk; a.sB = kk; a.ntaps = ntaps; a.scale = scale;
  for (int t = 0; t < ntaps && t < 25; ++t) a.tap_off[t] = t;
}

bool down_args(GatherArgs& a, const ConvGeom& g, int N, int Hl, int Wl, int Hs, int Ws, int ntaps) {
  std::memset(&a, 0, sizeof(a));
  if (ntaps <= 0) ntaps = g.k * g.k;
  if (ntaps > kMaxTaps || ntaps > g.k * g.k) return false;
  a.N = N; a.Hi = Hl; a.Wi = Wl; a.Cin = g.D1; a.Ho = Hs; a.Wo = Ws; a.Cout = g.D0; a.SI = g.s; a.SO = 1;
  a.gk = g.k; a.gs = g.s; a.gp = g.p; a.gup = 1;
  a.nphase = 1;
  a.phases[0] = Phase{0, 0, Hs, Ws, ntaps, 0, 0};
  for (int t = 0; t < ntaps; ++t) a.taps[t] = Tap{t / g.k - g.p, t % g.k - g.p};
  return true;
}
bool up_args(GatherArgs& a, const ConvGeom& g, int N, int Hs, int Ws, int Hl, int Wl, bool skip_empty) {
  std::memset(&a, 0, sizeof(a));
  if (g.s > 2 || g.k * g.k > kMaxTaps) return false;
  a.N = N; a.Hi = Hs; a.Wi = Ws; a.Cin = g.D0; a.Ho = Hl; a.Wo = Wl; a.Cout = g.D1; a.SI = 1; a.SO = g.s;
  a.gk = g.k; a.gs = g.s; a.gp = g.p; a.gup = 2;
  UpPhase ph[4];
  const int np = up_phases(g.k, g.s, g.p, ph);
  long off = 0; int tap0 = 0; a.nphase = 0;
  for (int i = 0; i < np; ++i) {
    const int Hq = Hl > ph[i].ph ? (Hl - ph[i].ph + g.s - 1) / g.s : 0;
    const int Wq = Wl > ph[i].pw ? (Wl - ph[i].pw + g.s - 1) / g.s : 0;
    const bool skip = (ph[i].ntaps == 0 && skip_empty) || Hq == 0 || Wq == 0;
    if (!skip) {
      a.phases[a.nphase++] = Phase{ph[i].ph, ph[i].pw, Hq, Wq, ph[i].ntaps, tap0, off};
      for (int t = 0; t < ph[i].ntaps; ++t) a.taps[tap0 + t] = Tap{ph[i].dh[t], ph[i].dw[t]};
      tap0 += ph[i].ntaps;
    }
    off += (long)g.D1 * ph[i].ntaps * g.D0;
  }
  return true;
}

// Asked of a one-image launch: a layer's layout is settled before any batch size is known, and the batch only enters the two kernels' conditions
// through their 32-bit offset limits.
static ConvLayout layout_of(int dt, GatherArgs& a) {
  ConvLayout r;
  if (a.nphase == 0) return r;
  a.wfrag = 1;
  r.frag = gather_deep2_takes(dt, dt, a);
  r.pos = gather_pos_takes(dt, dt, a);
  a.fp8 = 1;
  r.fp8 = gather_deep2_takes(dt, dt, a);
  return r;
}
ConvLayout op_down_layout(int dt, const ConvGeom& g, int Hl, int Wl) {
  GatherArgs a;
  if (!down_args(a, g, 1, Hl, Wl, conv_down_size(Hl, g.k, g.s, g.p), conv_down_size(Wl, g.k, g.s, g.p))) return ConvLayout();
  return layout_of(dt, a);
}
ConvLayout op_up_layout(int dt, const ConvGeom& g, int Hl, int Wl, int allow_empty_phases) {
  GatherArgs a;
  if (!up_args(a, g, 1, conv_down_size(Hl, g.k, g.s, g.p), conv_down_size(Wl, g.k, g.s, g.p), Hl, Wl, allow_empty_phases != 0)) return ConvLayout();
  return layout_of(dt, a);
}

// the prologue, statistics rows and accumulate of a launch's operands, its second source and the layout of its packed weights
static void set_operands(GatherArgs& a, const void* packed, const MapIn& in, const MapOut& out, const SecondSrc& x2) {
  if (x2.x2) { a.x2 = x2.x2; a.w2 = x2.w2; a.Cin2 = x2.Cin2; a.x2_ph = 0; a.x2_pw = 0; }
  a.fp8 = x2.fp8; a.wfrag = x2.wfrag; a.wfrag2 = x2.wfrag2;
  a.x = in.x; a.w = packed; a.y = out.y;
  a.pro_scale = in.pro.scale; a.pro_shift = in.pro.shift; a.pro_relu = in.relu; a.stats = out.stats; a.accumulate = out.accumulate;
}

int op_run_down(int dt, int out_dt, const ConvGeom& g, const void* packed, const MapIn& L, const MapOut& S, int N, hipStream_t s, const SecondSrc& x2) {
  GatherArgs a;
  if (!down_args(a, g, N, L.H, L.W, S.H, S.W)) { set_error("run_down: k=%d too large", g.k); return MMVAE_ERR_UNSUPPORTED; }
  set_operands(a, packed, L, S, x2);
  return launch_gather_gemm(dt, out_dt, a, s);
}

int op_run_up(int dt, const ConvGeom& g, const void* packed, const MapIn& S, const MapOut& L, int N, hipStream_t s, const SecondSrc& x2) {
  GatherArgs a;
  if (!up_args(a, g, N, S.H, S.W, L.H, L.W, L.accumulate != 0)) { set_error("run_up: k=%d s=%d unsupported", g.k, g.s); return MMVAE_ERR_UNSUPPORTED; }
  set_operands(a, packed, S, L, x2);
  if (a.nphase == 0) return 1;
  return launch_gather_gemm(dt, dt, a, s);
}

int op_run_wgrad(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, float* dW, int N, hipStream_t s, const WgradOpts& o) {
  if (g.k * g.k > 25) { set_error("wgrad: k=%d too large", g.k); return MMVAE_ERR_UNSUPPORTED; }
  if (o.defer) o.defer->nparts = 0;
  WgradArgs a;
  wgrad_args(a, g, N, P, G, dW, o.scratch, o.scale);
  a.defer = o.defer;
  return launch_wgrad(dt, a, s);
}

// A 3x3 stride-2 conv and the 1x1 stride-2 shortcut on the same input (a residual block's conv1 / downsample.0): both weight gradients from one
// pass over the block input.  Returns 1 when taken, 0 when the shapes are not the stream kernel's (the caller runs the two separately), <0 on error.
int op_run_wgrad_pair(int dt, const ConvGeom& g, const ConvGeom& gs, const MapIn& P, const void* P2, const MapIn& G, float* dW, float* dW2, int N,
                      hipStream_t s, const WgradOpts& o) {
  if (g.k != 3 || g.p != 1 || gs.k != 1 || gs.p != 0 || gs.s != g.s || gs.D0 != g.D0 || gs.D1 != g.D1) return 0;
  WgradArgs a;
  wgrad_args(a, g, N, MapIn(P.x, P.H, P.W), G, dW, o.scratch, o.scale);      // (no prologue on the dy side)
  return try_wgrad_stream_pair(dt, a, P2, dW2, o.scale2, s);
}

// The shape predicates: the launch's WgradArgs without data.  The kernels' conditions want a scratch (its address is not used).
static bool shape_args(WgradArgs& a, const ConvGeom& g, const MapIn& P, const MapIn& G, int N) {
  static float scratch = 0.f;
  if (g.k * g.k > 25) return false;
  wgrad_args(a, g, N, P, G, nullptr, &scratch);
  return true;
}
// whether op_run_wgrad runs this layer on the per-wave stream kernel (whose partial images are <= 19 MB and whose reduce can be deferred)
bool op_wgrad_is_stream(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, int N) {
  WgradArgs a;
  return shape_args(a, g, P, G, N) && wgrad_stream_shape(dt, a);
}
bool op_bwd_fusable(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, int N) {
  WgradArgs a;
  return shape_args(a, g, MapIn(nullptr, P.H, P.W), MapIn(nullptr, G.H, G.W), N) && dgrad_wgrad_stream_shape(dt, a);
}
// whether op_run_bwd_fused takes this layer with a join gradient `jg` (see kernels.hpp)
bool op_bwd_fusable_jg(int dt, const ConvGeom& g, const MapIn& P, const MapIn& G, int N, bool has_x2, bool bn_sums) {
  WgradArgs a;
  return shape_args(a, g, P, MapIn(nullptr, G.H, G.W), N) && dgrad_wgrad_stream_jg_shape(dt, a, has_x2, bn_sums);
}

int op_run_bwd_fused(int dt, const ConvGeom& g, const void* packed_down, const MapIn& P, const MapIn& G, const SecondSrc& x2, void* dP, float* dW, int N,
                     hipStream_t s, const WgradOpts& o) {
  if (g.k * g.k > 25) return 0;
  WgradArgs a;
  wgrad_args(a, g, N, P, MapIn(G.x, G.H, G.W), dW, o.scratch, o.scale);      // (G is a gradient: no prologue)
  a.M = a.N * a.Hp * a.Wp;
  return try_dgrad_wgrad_stream(dt, a, packed_down, dP, x2.x2, x2.w2, o.bn_part, s, o.dW2, o.scale2, o.jg);
}

int op_pack_flipped3(int dt, const float* w, void* dst, int Cin, int Cout, hipStream_t s, float scale) {
  PackArgs pf; std::memset(&pf, 0, sizeof(pf));
  pf.src = w; pf.dst = dst; pf.cols = Cin; pf.K = Cout; pf.ntaps = 9; pf.s_col = 9; pf.s_k = Cin * 9; pf.scale = scale;
  for (int t = 0; t < 9; ++t) pf.tap_off[t] = 8 - t;
  return launch_pack(dt, pf, s);
}

static inline int stem_cpad(int dt) { return dt == DT_F32 ? 4 : 8; }
int op_pack_stem(int dt, const float* w, int in_ch, void* dst, hipStream_t s) {
  PackArgs pa; std::memset(&pa, 0, sizeof(pa));
  pa.src = w; pa.dst = dst;
  pa.cols = 32; pa.K = stem_cpad(dt); pa.K_valid = in_ch; pa.ntaps = 25; pa.s_col = 25 * in_ch; pa.s_k = 25; pa.scale = 1.f;
  for (int t = 0; t < 25; ++t) pa.tap_off[t] = t;
  return launch_pack(dt, pa, s);
}
int op_run_stem(int dt, const void* packed, const void* x, int in_ch, int S, const MapOut& y, int N, hipStream_t s) {
  GatherArgs a;
  down_args(a, ConvGeom{32, stem_cpad(dt), 5, 2, 2}, N, S, S, y.H, y.W);
  a.x = x; a.w = packed; a.y = y.y; a.stats = y.stats;
  a.x_planar = 2; a.x_planes = in_ch;
  return launch_gather_gemm(dt, dt, a, s);
}

}  // namespace mmvae
