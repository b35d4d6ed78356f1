// Per-frame squared error and SSIM of n pairs of S x S planes (11 <= S <= 64), one launch, everything in f64.  Both sides are column
// descriptors of the contact sheet (mmvae_panel_col) and are reduced to bytes by panel_byte() of panel_decode.hpp -- the function the
// sheet kernel calls -- or taken as they are (MMVAE_FRAME_BYTES_U8): the metric is of exactly the bytes a sheet would show.  The rule
// (Wang et al. 2004, 11 x 11 Gaussian window of sigma 1.5, valid positions only) is spelled out in include/mmvae.h.
//
// Dataflow.  One block of 256 threads per plane pair; W = S - 10 valid positions per row and column.
//   stage:      every pixel of both planes is decoded once into two byte planes in LDS (2 x 4 KB at S = 64); (a - b)^2 is summed on the
//               way in 32-bit integers (at most 4096 * 65025 < 2^32), so the squared error is exact.
//   horizontal: a thread per (row y, valid column x) forms the 11-tap row sums of FOUR quantities -- a, b, a^2 + b^2, a b -- into LDS f64.
//               The formula needs sigma_a^2 + sigma_b^2 only as a sum, so E[a^2] and E[b^2] travel as one map.  The window is symmetric:
//               the taps k and 10 - k are added as integers first (exact), which halves the int -> f64 conversions and the multiplies.
//   vertical:   a thread per (group of 4 output rows, x) reads 14 rows of the four row sums once and forms 4 x 4 column sums in
//               registers (3.1 x fewer LDS reads than one output per thread), then the map value of its 4 positions.
//   The row sums live in a ring of 26 rows (16 output rows per step need 16 + 10): a step computes only the 16 rows it adds, no row sum is
//   formed twice, and the f64 buffer stays at 26 * 4 * 54 * 8 = 44 928 B.  With the byte planes: 53 120 B of LDS, three blocks per CU.
//   reduce:     per-thread partial sums of the map (fixed assignment of positions to threads), then a fixed binary tree over the 256
//               threads in LDS (the ring is dead by then and is reused).  No atomics: the same bits every run.
// LDS layout of the ring is [slot][quantity][x]: neighbouring lanes are neighbouring x in both passes, so every f64 access is a run of
// consecutive 8-byte words (conflict-free); neighbouring lanes of the byte reads share dwords (broadcast).
#include <math.h>

#include "common.hpp"
#include "kernels.hpp"
#include "panel_decode.hpp"

namespace mmvae {

namespace {

constexpr int kThreads = 256;
constexpr int kMinS = 11, kMaxS = 64;
constexpr int kTaps = 11, kHalf = 5;
constexpr int kMaxW = kMaxS - (kTaps - 1);                           // 54 valid positions per row
constexpr int kBand = 16;                                            // output rows per step
constexpr int kRing = kBand + kTaps - 1;                             // 26 rows of row sums resident
constexpr int kRowsPerThread = 4;                                    // output rows of one thread of the vertical pass
constexpr int kSpan = kRowsPerThread + kTaps - 1;                    // 14 rows it reads
constexpr int kQty = 4;                                              // a, b, a^2 + b^2, a b
static_assert(kBand / kRowsPerThread * kMaxW <= kThreads, "the vertical pass is one round of the block");
static_assert(kThreads * (sizeof(double) + sizeof(unsigned)) <= kRing * kQty * kMaxW * sizeof(double), "the reduction reuses the ring");

struct Window { double g[kTaps]; };

__device__ __forceinline__ unsigned side_byte(const mmvae_panel_col& col, long r, int pix, int HW) {
  if (col.kind == MMVAE_FRAME_BYTES_U8) return static_cast<const unsigned char*>(col.src)[r * HW + pix];
  return panel_byte(col, r, pix, HW);
}

// one position of the SSIM map from the four windowed means
__device__ __forceinline__ double ssim_value(double ma, double mb, double e2, double eab) {
  constexpr double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double mab = ma * mb, m2 = ma * ma + mb * mb;
  return ((2.0 * mab + C1) * (2.0 * (eab - mab) + C2)) / ((m2 + C1) * ((e2 - m2) + C2));
}

__global__ __launch_bounds__(kThreads) void frame_quality_kernel(mmvae_panel_col ca, mmvae_panel_col cb, Window win, int n, int S,
                                                                double* __restrict__ out) {
  __shared__ unsigned char pa[kMaxS * kMaxS], pb[kMaxS * kMaxS];
  __shared__ double ring[kRing * kQty * kMaxW];
  const long r = blockIdx.x;                                         // the plane pair
  const int tid = threadIdx.x;
  const int HW = S * S, W = S - (kTaps - 1);

  unsigned sse = 0;
  for (int pix = tid; pix < HW; pix += kThreads) {
    const unsigned a = side_byte(ca, r, pix, HW), b = side_byte(cb, r, pix, HW);
    pa[pix] = (unsigned char)a;
    pb[pix] = (unsigned char)b;
    const int d = (int)a - (int)b;
    sse += (unsigned)(d * d);
  }
  __syncthreads();

  double acc = 0.0;
  for (int r0 = 0; r0 < W; r0 += kBand) {                            // output rows [r0, r0 + 16) need row sums of rows [r0, r0 + 26)
    const int y_begin = r0 == 0 ? 0 : r0 + kTaps - 1;                // the rows below are in the ring already
    const int y_end = min(r0 + kRing, S);
    for (int i = tid; i < (y_end - y_begin) * W; i += kThreads) {
      const int dy = i / W, x = i - dy * W, y = y_begin + dy;
      const unsigned char* __restrict__ ra = pa + y * S + x;
      const unsigned char* __restrict__ rb = pb + y * S + x;
      const int ac = ra[kHalf], bc = rb[kHalf];
      double h0 = win.g[kHalf] * (double)ac, h1 = win.g[kHalf] * (double)bc;
      double h2 = win.g[kHalf] * (double)(ac * ac + bc * bc), h3 = win.g[kHalf] * (double)(ac * bc);
#pragma unroll
      for (int k = 0; k < kHalf; ++k) {                              // taps k and 10 - k share a weight: add them as integers, exactly
        const int a0 = ra[k], a1 = ra[kTaps - 1 - k], b0 = rb[k], b1 = rb[kTaps - 1 - k];
        h0 = fma(win.g[k], (double)(a0 + a1), h0);
        h1 = fma(win.g[k], (double)(b0 + b1), h1);
        h2 = fma(win.g[k], (double)(a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1), h2);
        h3 = fma(win.g[k], (double)(a0 * b0 + a1 * b1), h3);
      }
      double* dst = ring + (y % kRing) * (kQty * W) + x;
      dst[0] = h0;
      dst[W] = h1;
      dst[2 * W] = h2;
      dst[3 * W] = h3;
    }
    __syncthreads();
    if (tid < (kBand / kRowsPerThread) * W) {
      const int j = tid / W, x = tid - j * W;
      const int o0 = r0 + kRowsPerThread * j;                        // first output row of this thread
      if (o0 < W) {
        double v[kRowsPerThread][kQty];
#pragma unroll
        for (int o = 0; o < kRowsPerThread; ++o)
#pragma unroll
          for (int q = 0; q < kQty; ++q) v[o][q] = 0.0;
#pragma unroll
        for (int dr = 0; dr < kSpan; ++dr) {
          const int y = o0 + dr;
          if (y < S) {                                               // a row past the plane feeds only outputs past W, which are dropped
            const double* src = ring + (y % kRing) * (kQty * W) + x;
            const double s0 = src[0], s1 = src[W], s2 = src[2 * W], s3 = src[3 * W];
#pragma unroll
            for (int o = 0; o < kRowsPerThread; ++o) {
              const int k = dr - o;
              if (k >= 0 && k < kTaps) {
                v[o][0] = fma(win.g[k], s0, v[o][0]);
                v[o][1] = fma(win.g[k], s1, v[o][1]);
                v[o][2] = fma(win.g[k], s2, v[o][2]);
                v[o][3] = fma(win.g[k], s3, v[o][3]);
              }
            }
          }
        }
#pragma unroll
        for (int o = 0; o < kRowsPerThread; ++o)
          if (o0 + o < W) acc += ssim_value(v[o][0], v[o][1], v[o][2], v[o][3]);
      }
    }
    __syncthreads();                                                 // the next step overwrites the 16 oldest rows of the ring
  }

  double* red = ring;                                                // the ring is dead: a fixed tree over the block
  unsigned* red_u = reinterpret_cast<unsigned*>(ring + kThreads);
  red[tid] = acc;
  red_u[tid] = sse;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red_u[tid] += red_u[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[r] = (double)red_u[0];
    out[(long)n + r] = red[0] / (double)(W * W);
  }
}

int check_side(const mmvae_panel_col& k, const char* side) {
  if (k.kind < MMVAE_PANEL_LABELS_U8 || k.kind > MMVAE_FRAME_BYTES_U8) { set_error("frame_quality: side %s has kind %d", side, k.kind); return MMVAE_ERR_ARG; }
  if (!k.src) { set_error("frame_quality: side %s has no source", side); return MMVAE_ERR_ARG; }
  if (k.kind == MMVAE_FRAME_BYTES_U8) return MMVAE_OK;
  if (k.kind == MMVAE_PANEL_IMAGE_F32) {
    if (!(k.hi > k.lo)) { set_error("frame_quality: side %s needs hi > lo", side); return MMVAE_ERR_ARG; }
    return MMVAE_OK;
  }
  if (k.Q < 1 || k.Q > kPanelMaxQ) { set_error("frame_quality: side %s has Q=%d (1..%d)", side, k.Q, kPanelMaxQ); return MMVAE_ERR_ARG; }
  if (!k.lut) { set_error("frame_quality: side %s has no lut", side); return MMVAE_ERR_ARG; }
  if (k.kind == MMVAE_PANEL_LOGITS_SAMPLE && !k.uniforms) { set_error("frame_quality: side %s samples without uniforms", side); return MMVAE_ERR_ARG; }
  return MMVAE_OK;
}

Window make_window() {
  Window w;
  double sum = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    w.g[k] = exp(-(double)((k - kHalf) * (k - kHalf)) / (2.0 * 1.5 * 1.5));
    sum += w.g[k];
  }
  for (int k = 0; k < kTaps; ++k) w.g[k] /= sum;
  return w;
}

}  // namespace

int launch_frame_quality(const mmvae_panel_col* a, const mmvae_panel_col* b, int n, int S, double* out, hipStream_t s) {
  if (!a || !b || !out) { set_error("frame_quality: NULL a, b or out"); return MMVAE_ERR_ARG; }
  if (n < 1) { set_error("frame_quality: n=%d must be positive", n); return MMVAE_ERR_ARG; }
  if (int rc = check_side(*a, "a")) return rc;
  if (int rc = check_side(*b, "b")) return rc;
  if (S < kMinS || S > kMaxS) { set_error("frame_quality: S=%d unsupported (%d..%d: an 11 x 11 window, planes of at most 64 x 64)", S, kMinS, kMaxS); return MMVAE_ERR_UNSUPPORTED; }
  static const Window win = make_window();                           // the eleven weights, once, in double on the host
  hipLaunchKernelGGL(frame_quality_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, *a, *b, win, n, S, out);
  return check_launch("frame_quality");
}

}  // namespace mmvae
