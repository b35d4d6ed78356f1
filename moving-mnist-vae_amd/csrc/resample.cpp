// Coefficient tables of the device resize (resize.hip): the reference's transforms.Resize (main.py:33-36) is Pillow's 8-bit
// antialiased bilinear resample, and a label next to a k-means boundary moves with a byte that is off by one, so the tables repeat
// Pillow's precompute_coeffs / normalize_coeffs_8bpc operation by operation: everything in f64, the triangle filter stretched by
// the shrink factor, the weights of one output summed in index order and DIVIDED by that sum, then rounded to 22-bit fixed point.
// Plain C++: no HIP header.  Built with -ffp-contract=off (Makefile) and the pragma below, never with fast-math: a fused
// multiply-add or a reciprocal in place of the division changes a coefficient's last bit and with it a byte.
//
// A pass that uses the tables computes out = clamp((2^21 + sum_x pixel[first + x] * k[x]) >> 22, 0, 255) in int32: the taps of an
// output sum to 2^22 +- ksize, so the largest sum is 255 * (2^22 + ksize) + 2^21 < 2^31.
#include "resample.hpp"

#include <math.h>

#include "../../include/mmvae.h"

#ifdef __FAST_MATH__
#error "resample.cpp repeats Pillow's f64 arithmetic: build it without fast-math"
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace mmvae {

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;     // 22

inline double triangle(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

}  // namespace

int resample_coeffs(int in_size, int out_size, int* ksize_out, int32_t* bounds, int32_t* coeffs) {
  if (in_size < 1 || in_size > kResampleMaxSize || out_size < 1 || out_size > kResampleMaxSize) {
    set_error("resample_coeffs: sizes %d -> %d outside [1, %d]", in_size, out_size, kResampleMaxSize);
    return MMVAE_ERR_ARG;
  }
  if (!ksize_out) { set_error("resample_coeffs: NULL ksize"); return MMVAE_ERR_ARG; }
  if ((bounds == nullptr) != (coeffs == nullptr)) { set_error("resample_coeffs: bounds and coeffs must both be given or both be NULL"); return MMVAE_ERR_ARG; }
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  *ksize_out = ksize;
  if (!bounds) return MMVAE_OK;
  double w[2 * kResampleMaxSize + 1];
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;                  // <= ksize
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = triangle((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int32_t* k = coeffs + (long)xx * ksize;
    for (int x = 0; x < n; ++x) {
      if (ww != 0.0) w[x] /= ww;
      k[x] = w[x] < 0 ? (int32_t)(-0.5 + w[x] * (1 << kPrecisionBits)) : (int32_t)(0.5 + w[x] * (1 << kPrecisionBits));
    }
    for (int x = n; x < ksize; ++x) k[x] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  return MMVAE_OK;
}

}  // namespace mmvae
